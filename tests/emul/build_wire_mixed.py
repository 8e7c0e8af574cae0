"""Builds the TEST-ONLY forms of the mixed-value-count wire expansion (bp_pp_amd/csrc/wire_mixed_core.h, k_wire_mixed.hip):
    "host"    tests/emul/wire_mixed_emul.cpp with g++: the lane function over every lane, behind guard pages
    "gfx950"  tests/emul/wire_mixed_device.hip with hipcc: the product's kernel unit as it is plus a C runner over device pointers"""
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
SO = {"host": os.path.join(HERE, "libbppp_wire_mixed_emul.so"), "gfx950": os.path.join(HERE, "libbppp_wire_mixed_hip.so")}
SRC = {"host": "wire_mixed_emul.cpp", "gfx950": "wire_mixed_device.hip"}


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def build(backend):
    so, src = SO[backend], os.path.join(HERE, SRC[backend])
    csrc = os.path.join(ROOT, "bp_pp_amd", "csrc")
    deps = [src] + glob.glob(os.path.join(csrc, "*.h")) + ([os.path.join(csrc, "k_wire_mixed.hip")] if backend == "gfx950" else [])
    if os.path.exists(so) and not any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        return so
    tmp = so + ".tmp%d" % os.getpid()
    if backend == "host":
        cmd = ["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", tmp, src]
    else:
        from bp_pp_amd._build import BASE_FLAGS
        cmd = [_hipcc(), *BASE_FLAGS, "-shared", "-Wl,-rpath,/opt/rocm/lib", "-o", tmp, src]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building %s failed:\n%s" % (os.path.basename(so), r.stderr[-6000:]))
    os.replace(tmp, so)
    return so


def build_all():
    """What __graft_entry__.build() calls (the gfx950 form cross-compiles without a GPU)."""
    return [build(b) for b in SO if b == "host" or os.path.exists(_hipcc())]


def load(backend="host"):
    L = C.CDLL(build(backend))
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    if backend == "host":
        L.emul_wire_mixed_lanes.argtypes = [sz, i32, i32, i32]
        L.emul_wire_mixed_lanes.restype = C.c_ulonglong
        L.emul_wire_expand_mixed.argtypes = [vp, sz, vp, sz, vp, vp, vp, sz, i32, i32, i32, i32]
        L.emul_wire_expand_mixed.restype = i32
    else:
        L.wire_mixed_run_device.argtypes = [vp, vp, vp, vp, vp, sz, i32, i32, i32]
        L.wire_mixed_run_device.restype = i32
    return L
