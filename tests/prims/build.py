"""Builds the TEST-ONLY primitive libraries of tests/test_prims*.py from one dispatcher (prims_core.h):

  libbppp_prims_gcc.so    g++ host build (prims_host.cpp): the code path of the tests/emul emulation
  libbppp_prims_clang.so  ROCm's clang++ host build (prims_host.cpp): field.h's __builtin_addc / __builtin_subc carry chains
  libbppp_prims_hip.so    hipcc gfx950 build (prims_device.hip, bucket_device.hip, agg_device.hip, circuit_device.hip) with the product's
                          BASE_FLAGS: the code the GPU runs

Each library exports the dispatcher (prims_run_host / prims_run_device) and the variable-base sums (prims_run_sums_host: the one-lane
forms; prims_run_sums_device: those and the lane-group forms) and the transcript primitives (prims_run_transcript_host: the register
sponge; prims_run_transcript_device: that and the LDS sponge, in the uniform and the grouped launch layout) and the bucket stage of the
RLC batch mode (tests/test_prims_bucket.py, arguments in bucket_prims.h; prims_run_bucket_host: the single-thread form of bucket_core.h;
prims_run_bucket_device: the product's own k_bkt_* kernels, whose translation unit bucket_device.hip includes as it is) and the
aggregated range proof's phase 1, C0 stage and prover stages (tests/test_prims_agg.py, arguments in agg_prims.h;
prims_run_agg_verify_host / prims_run_agg_prove_host: the single-thread forms; prims_run_agg_*_device: the product's own k_agg_* and
k_aprove_* kernels, whose translation units agg_device.hip includes as they are) and the generic circuit verifier's phase 1 and C0
stage (tests/test_prims_circuit.py, arguments in circuit_prims.h; prims_run_circuit_host: the single-thread form; prims_run_circuit_device:
the product's own k_circuit_* kernels, circuit_device.hip includes k_generic.hip as it is; prims_circuit_plan, host builds: plan_generic's
choices for a circuit call).  A library is
rebuilt when it is missing or older than any bp_pp_amd/csrc/*.h, an included kernel unit or any tests/prims/* source."""
import ctypes as C
import glob
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BACKENDS = ("gcc", "clang", "gfx950")
SO = {
    "gcc": os.path.join(HERE, "libbppp_prims_gcc.so"),
    "clang": os.path.join(HERE, "libbppp_prims_clang.so"),
    "gfx950": os.path.join(HERE, "libbppp_prims_hip.so"),
}
HOST_FLAGS = ["-O2", "-shared", "-fPIC", "-std=c++17"]
DEVICE_UNITS = ("prims_device.hip", "bucket_device.hip", "agg_device.hip", "circuit_device.hip")
# bp_pp_amd/csrc units that bucket_device.hip, agg_device.hip and circuit_device.hip include
INCLUDED_KERNEL_UNITS = ("k_verify_bucket.hip", "k_agg.hip", "k_aggprove.hip", "k_generic.hip")


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def clangxx():
    """ROCm's LLVM clang++, found next to hipcc; None if it is not there."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(_hipcc())))
    for cand in (os.path.join(rocm, "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(cand):
            return cand
    return None


def _stale(so):
    csrc = os.path.join(ROOT, "bp_pp_amd", "csrc")
    deps = glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(csrc, u) for u in INCLUDED_KERNEL_UNITS] + [
        p for p in glob.glob(os.path.join(HERE, "*")) if os.path.isfile(p) and not p.endswith(".so") and "__pycache__" not in p]
    return not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps)


def unavailable(backend):
    """Why `backend` cannot be built here, or None."""
    if backend == "clang" and clangxx() is None:
        return "ROCm's clang++ (llvm/bin/clang++ beside hipcc) is not installed"
    if backend == "gfx950" and not os.path.exists(_hipcc()):
        return "hipcc is not installed"
    return None


def build(backend, force=False):
    so = SO[backend]
    if not force and not _stale(so):
        return so
    why = unavailable(backend)
    if why:
        raise RuntimeError(why)
    if backend == "gfx950":
        return _build_device(so)
    cxx = "g++" if backend == "gcc" else clangxx()
    cmd = [cxx, *HOST_FLAGS, "-o", so + ".tmp", os.path.join(HERE, "prims_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building {os.path.basename(so)} failed:\n{r.stderr[-6000:]}")
    os.replace(so + ".tmp", so)
    return so


def _build_device(so):
    """The device units side by side, one hipcc -c each (a unit that includes a product kernel unit takes minutes, and one command
    compiles its inputs one after the other), then one link.  The objects live in a temporary directory."""
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    from bp_pp_amd._build import BASE_FLAGS
    with tempfile.TemporaryDirectory(prefix="bppp_prims_") as tmp:
        def compile_one(unit):
            obj = os.path.join(tmp, unit[:-4] + ".o")
            r = subprocess.run([_hipcc(), *BASE_FLAGS, "-c", os.path.join(HERE, unit), "-o", obj], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"building {os.path.basename(so)} failed on {unit}:\n{r.stderr[-6000:]}")
            return obj
        with ThreadPoolExecutor(max_workers=min(len(DEVICE_UNITS), os.cpu_count() or 1)) as ex:
            objs = list(ex.map(compile_one, DEVICE_UNITS))
        r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-rpath,/opt/rocm/lib", "-o", so + ".tmp", *objs],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"linking {os.path.basename(so)} failed:\n{r.stderr[-6000:]}")
    os.replace(so + ".tmp", so)
    return so


def build_all():
    """What __graft_entry__.build() calls: every backend that can be built here (the gfx950 one cross-compiles without a GPU)."""
    return [build(b) for b in BACKENDS if unavailable(b) is None]


def load(backend):
    L = C.CDLL(build(backend))
    vp, sz = C.c_void_p, C.c_size_t
    L.prims_record_words.argtypes = [C.c_int]
    L.prims_record_words.restype = C.c_int
    run = L.prims_run_device if backend == "gfx950" else L.prims_run_host
    run.argtypes = [vp, vp, sz, vp, sz]
    run.restype = C.c_int
    L.run = run
    L.prims_sum_words.argtypes = [C.c_int]
    L.prims_sum_words.restype = C.c_int
    run_sums = L.prims_run_sums_device if backend == "gfx950" else L.prims_run_sums_host
    run_sums.argtypes = [C.c_uint32, vp, vp, sz]
    run_sums.restype = C.c_int
    L.run_sums = run_sums
    L.prims_transcript_words.argtypes = [C.c_int]
    L.prims_transcript_words.restype = C.c_int
    run_tr = L.prims_run_transcript_device if backend == "gfx950" else L.prims_run_transcript_host
    run_tr.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, sz]
    run_tr.restype = C.c_int
    L.run_transcript = run_tr
    u64p = C.POINTER(C.c_uint64)
    L.prims_bucket_fb_entries.argtypes = [C.c_int, C.c_int]
    L.prims_bucket_fb_entries.restype = sz
    L.prims_bucket_fb_build.argtypes = [C.c_char_p, C.c_int, C.c_int, vp]
    L.prims_bucket_fb_build.restype = C.c_int
    L.prims_bucket_geometry.argtypes = [C.c_uint32, C.c_int, u64p]
    L.prims_bucket_geometry.restype = None
    run_bkt = L.prims_run_bucket_device if backend == "gfx950" else L.prims_run_bucket_host
    run_bkt.argtypes = [sz, C.c_uint32, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    run_bkt.restype = C.c_int
    L.run_bucket = run_bkt
    for name in ("verify", "prove"):
        fn = getattr(L, f"prims_run_agg_{name}_" + ("device" if backend == "gfx950" else "host"))
        fn.argtypes = [vp, vp, vp]
        fn.restype = C.c_int
        setattr(L, f"run_agg_{name}", fn)
    run_circ = L.prims_run_circuit_device if backend == "gfx950" else L.prims_run_circuit_host
    run_circ.argtypes = [vp, vp, vp]
    run_circ.restype = C.c_int
    L.run_circuit = run_circ
    if backend != "gfx950":
        L.prims_is_clang.restype = C.c_int
        L.prims_circuit_plan.argtypes = [sz, sz, sz, C.c_int, C.c_int, vp]
        L.prims_circuit_plan.restype = None
    return L
