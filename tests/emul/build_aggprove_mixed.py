"""Builds the TEST-ONLY host emulation of the mixed-value-count aggregate prover's device code (tests/emul/aggprove_mixed_emul.cpp) with g++."""
import ctypes as C
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SO = os.path.join(HERE, "libbppp_aggprove_mixed_emul.so")


def load():
    src = os.path.join(HERE, "aggprove_mixed_emul.cpp")
    deps = [src] + glob.glob(os.path.join(ROOT, "bp_pp_amd", "csrc", "*.h"))
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = SO + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", tmp, src])
        os.replace(tmp, SO)
    L = C.CDLL(SO)
    vp, sz, i32, cp = C.c_void_p, C.c_size_t, C.c_int, C.c_char_p
    L.emul_aggprove_mixed_args_ok.argtypes = [sz, sz, sz, sz, vp, i32, sz, sz]
    L.emul_aggprove_mixed.argtypes = [vp, i32, i32, i32, i32, i32, i32, cp, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    return L
