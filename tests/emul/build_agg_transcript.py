"""Builds the TEST-ONLY host emulation of the aggregate's caller-transcript device code (tests/emul/agg_transcript_emul.cpp) with g++."""
import ctypes as C
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SO = os.path.join(HERE, "libbppp_agg_transcript_emul.so")


def load():
    src = os.path.join(HERE, "agg_transcript_emul.cpp")
    deps = [src] + glob.glob(os.path.join(ROOT, "bp_pp_amd", "csrc", "*.h"))
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = SO + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", tmp, src])
        os.replace(tmp, SO)
    L = C.CDLL(SO)
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    L.emul_aggtx_draws.argtypes = [sz, sz]
    L.emul_aggtx_draws.restype = sz
    L.emul_aggtx_position_key.argtypes = [vp, sz, sz]
    L.emul_aggtx_position_key.restype = C.c_uint
    L.emul_aggtx_verify.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, sz, sz, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.emul_aggtx_verify.restype = i32
    L.emul_aggtx_prove.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, sz, sz, vp, vp, vp, vp, vp, vp, vp]
    L.emul_aggtx_prove.restype = i32
    return L
