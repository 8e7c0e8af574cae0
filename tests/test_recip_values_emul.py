"""CPU tier for the reciprocal prover from integers (include/bppp.h: bppp_reciprocal_prove_values_batch*): the witness core
(bp_pp_amd/csrc/recip_witness_core.h, the code of k_rprove_witness) built with g++ and compared with plain Python big-integer
arithmetic -- digits, multiplicities and statuses -- and the admissibility rule dim_np^dim_nd <= n in its two copies (the library's
recip_values_shape_ok and bp_pp_amd.wnla.values_shape_ok)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
ST_BAD_ENCODING, ST_OUT_OF_RANGE = 1, 4
SHAPES = [(8, 4), (12, 10), (16, 16), (32, 16), (63, 16), (255, 2)]

SHIM = r'''
#include <cstdint>
#include <cstring>
#include "recip_witness_core.h"
using namespace bppp;
extern "C" {
// n instances: x n x 32 -> digits n x nd x 32, m n x np x 32, status n; returns 0
int rw_run(size_t n, int nd, int np, const uint8_t* x, uint8_t* digits, uint8_t* m, int32_t* status) {
    RecipWitnessWs w;
    std::memset(&w, 0, sizeof w);
    recip_witness_shape(w, (size_t)nd, (size_t)np);
    w.N = n; w.x = x; w.digits = digits; w.m = m; w.status = status;
    for (size_t t = 0; t < n; t++)
        if (recip_witness(w, t) != status[t]) return 1;
    return 0;
}
int rw_shape_ok(size_t nd, size_t np) { return recip_values_shape_ok(nd, np) ? 1 : 0; }
int rw_bits(size_t nd, size_t np) { RecipWitnessWs w; recip_witness_shape(w, nd, np); return w.bits; }
}
'''


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("recip_values")
    src, so = d / "rw_shim.cpp", d / "librw_shim.so"
    src.write_text(SHIM)
    r = subprocess.run([gxx, "-std=c++17", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "bp_pp_amd", "csrc"), str(src), "-o", str(so)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(str(so))
    L.rw_run.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rw_shape_ok.argtypes = [C.c_size_t, C.c_size_t]
    L.rw_bits.argtypes = [C.c_size_t, C.c_size_t]
    return L


def _values(nd, npp):
    top = npp ** nd
    xs = [0, 1, top - 1, top, top + 1, N - 1, N, (1 << 256) - 1]
    xs += [sum(v * npp ** i for i in range(nd)) for v in sorted({1, npp // 2, npp - 1})]          # every digit equal
    xs += [npp ** (nd - 1), npp ** (nd - 1) - 1, top - npp, (top - 1) // 2]                       # carries across every digit
    rng = np.random.default_rng(1000 * nd + npp)
    raw = [int.from_bytes(rng.bytes(32), "big") for _ in range(300)]
    xs += [v % top for v in raw[:200]] + raw[200:250] + [v % N for v in raw[250:]]               # in range | any 256 bits | canonical
    return [x for x in xs if 0 <= x < 1 << 256]


def _expected(x, nd, npp):
    digits = [(x // npp ** i) % npp for i in range(nd)]
    m = [digits.count(v) for v in range(npp)]
    status = ST_BAD_ENCODING if x >= N else (ST_OUT_OF_RANGE if x >= npp ** nd else 0)
    return digits, m, status


@pytest.mark.parametrize("nd,npp", SHAPES)
def test_witness_core_equals_big_integer_arithmetic(core, nd, npp):
    """Digits least significant first, multiplicities and status of every chosen value: 0, 1, np^nd - 1, np^nd, np^nd + 1, n - 1, n,
    2^256 - 1, all digits equal, and 300 pseudo-random ones.  (12, 10) takes the division path, the others the shifts.  A flagged
    value still gets the low nd digits of its 256-bit value and their counts: valid scalars for the stages behind the kernel."""
    assert (core.rw_bits(nd, npp) < 0) == (npp & (npp - 1) != 0)
    xs = _values(nd, npp)
    n = len(xs)
    X = np.frombuffer(b"".join(x.to_bytes(32, "big") for x in xs), np.uint8).reshape(n, 32).copy()
    D, M = np.full((n, nd, 32), 0xAA, np.uint8), np.full((n, npp, 32), 0xAA, np.uint8)
    st = np.full(n, 77, np.int32)
    assert core.rw_run(n, nd, npp, X.ctypes.data, D.ctypes.data, M.ctypes.data, st.ctypes.data) == 0
    seen = set()
    for i, x in enumerate(xs):
        digits, m, status = _expected(x, nd, npp)
        got_d = [int.from_bytes(D[i, j].tobytes(), "big") for j in range(nd)]
        got_m = [int.from_bytes(M[i, v].tobytes(), "big") for v in range(npp)]
        assert got_d == digits, hex(x)
        assert got_m == m and sum(got_m) == nd, hex(x)
        assert int(st[i]) == status, hex(x)
        seen.add(status)
    assert seen == {0, ST_BAD_ENCODING, ST_OUT_OF_RANGE}


def test_division_path_at_every_small_base(core):
    """The reciprocal-multiplication step (rw_next_digit) at every dim_np up to 48 -- past the largest an admissible shape with
    dim_np <= dim_nd + 1 can have -- and at the largest the entry points let through (4097), on values that put every limb at its
    extremes."""
    rng = np.random.default_rng(5)
    base = [0, 1, (1 << 256) - 1, N - 1, N, 1 << 255, (1 << 224) - 1, int("f" * 8 + "0" * 8, 16) * ((1 << 256) // ((1 << 64) - 1))]
    base += [int.from_bytes(rng.bytes(32), "big") for _ in range(40)]
    for npp in list(range(1, 49)) + [255, 257, 1000, 4095, 4097]:
        nd = 6
        n = len(base)
        X = np.frombuffer(b"".join(x.to_bytes(32, "big") for x in base), np.uint8).reshape(n, 32).copy()
        D, M, st = np.zeros((n, nd, 32), np.uint8), np.zeros((n, npp, 32), np.uint8), np.zeros(n, np.int32)
        assert core.rw_run(n, nd, npp, X.ctypes.data, D.ctypes.data, M.ctypes.data, st.ctypes.data) == 0
        for i, x in enumerate(base):
            digits, m, status = _expected(x, nd, npp)
            assert [int.from_bytes(D[i, j].tobytes(), "big") for j in range(nd)] == digits, (npp, hex(x))
            assert [int.from_bytes(M[i, v].tobytes(), "big") for v in range(npp)] == m, (npp, hex(x))
            assert int(st[i]) == status, (npp, hex(x))


ADMISSIBLE = [((63, 16), True), ((64, 16), False), ((255, 2), True), ((256, 2), False), ((77, 10), True), ((78, 10), False),
              ((8, 4), True), ((12, 10), True), ((16, 16), True), ((32, 16), True), ((256, 16), False), ((1, 1), True), ((4096, 1), True),
              ((46, 47), True), ((47, 47), False), ((0, 16), False), ((16, 0), False)]


@pytest.mark.parametrize("shape,ok", ADMISSIBLE)
def test_admissible_shapes(core, shape, ok):
    """dim_np^dim_nd <= n: 16^63, 2^255 and 10^77 are accepted, 16^64, 2^256 and 10^78 refused -- by the pure Python rule and by the
    library's copy of it, which must agree with each other and with the integers."""
    from bp_pp_amd.wnla import GROUP_ORDER, values_shape_ok
    nd, npp = shape
    assert GROUP_ORDER == N
    if nd and npp:
        assert (npp ** nd <= N) == ok
    assert values_shape_ok(nd, npp) == ok
    assert bool(core.rw_shape_ok(nd, npp)) == ok


def test_the_two_copies_of_the_rule_agree_on_a_grid(core):
    from bp_pp_amd.wnla import values_shape_ok
    for npp in list(range(1, 70)) + [255, 256, 257, 4097, 65535]:
        for nd in list(range(1, 70)) + [77, 78, 127, 128, 129, 255, 256, 257, 4096]:
            assert bool(core.rw_shape_ok(nd, npp)) == values_shape_ok(nd, npp), (nd, npp)


def test_new_entry_points_are_declared_bound_and_refuse_bad_arguments_without_a_gpu():
    """The four symbols in include/bppp.h, the binding and the built library; a NULL context is BPPP_ERR_INVALID_ARG."""
    from bp_pp_amd import _build, _capi
    text = open(os.path.join(ROOT, "include", "bppp.h")).read()
    assert "#define BPPP_ST_OUT_OF_RANGE 4" in text and _capi.ST_OUT_OF_RANGE == 4
    for name in _capi.VALUES_EXPORTS:
        assert name in _capi.EXPORTS and f"{name}(" in text
    if not os.path.exists(_build.SO):
        pytest.skip("libbppp_hip.so not built yet")
    L = _capi.lib()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    E = _capi.ERR_INVALID_ARG
    assert L.bppp_reciprocal_prove_values_batch(None, b"x", 1, 1, 8, 4, p, p, p, p, p, p) == E
    assert L.bppp_reciprocal_prove_values_batch_seeded(None, b"x", 1, 1, 8, 4, p, p, bytes(32), 0, p, p, p) == E
    assert L.bppp_reciprocal_prove_values_batch_device(None, b"x", 1, 1, 8, 4, p, p, p, p, p, p) == E
    assert L.bppp_reciprocal_prove_values_batch_seeded_device(None, b"x", 1, 1, 8, 4, p, p, bytes(32), 0, p, p, p) == E
