"""CPU tier for the aggregated reciprocal range proof PROVER's device code (bp_pp_amd/csrc/agg_prove_core.h and the generic circuit /
WNLA prover stages behind it, compiled for the host: tests/emul/aggprove_emul.cpp), one "thread" after the other:

  * the whole chain -- witness, value commitments, stage r1, pole commitments, stage r2, the circuit prover with the closed-form collect,
    the WNLA prover, the assembly -- against the oracle's bytes in tests/golden/agg_cases.json for every golden instance of the small
    shapes (instance 0 is all-zero digits, instance 1 all np - 1), and one instance of (16, 16, 16) (half a second on the host; its
    4-bit table over 289 generators a few seconds more);
  * the closed forms of lambda_vec, mu_vec and the six coefficient vectors against circuit_collect's walk over the explicit pattern,
    word for word ((6, 2, 3) has np = nd + 1);
  * the witness against Python big integers at the ends of the range, above it, at n - 1 and n, and a non-canonical s;
  * the argument rules on a grid."""
import hashlib

import numpy as np
import pytest

import agg_cases as A
import agg_golden
import agg_prove_cases as AP
from emul.build import load as load_emul
from emul.build_aggprove import load as load_aggprove

W = 4
SMALL = [(2, 4, 4), (3, 4, 4), (6, 2, 3), (7, 3, 4)]
ST_BAD_ENCODING, ST_OUT_OF_RANGE = 1, 4
_tables = {}


def _table(case):
    key = (case["k"], case["nd"])
    if key not in _tables:
        L = load_emul()
        gens = agg_golden.generators(case)
        NB = 1 + case["NG"] + case["NH"]
        tab = np.zeros(L.emul_fb_table_entries(NB, W) * 64, dtype=np.uint8)
        assert L.emul_fb_build(gens, NB, W, tab.ctypes.data) == 0
        _tables[key] = tab
    return _tables[key]


def _prove(case, x, s, rnd):
    L = load_aggprove()
    n, k = x.shape[0], case["k"]
    x, s, rnd = (np.ascontiguousarray(a) for a in (x, s, rnd))
    proofs = np.full((n, case["proof_bytes"]), 0xEE, np.uint8)
    com = np.full((n, k, 64), 0xEE, np.uint8)
    st = np.full(n, 7, np.int32)
    tab = _table(case)
    rc = L.emul_aggprove(tab.ctypes.data, W, case["NG"], case["NH"], k, case["nd"], case["np"], case["label"], len(case["label"]), n,
                         x.ctypes.data, s.ctypes.data, rnd.ctypes.data, proofs.ctypes.data, com.ctypes.data, st.ctypes.data)
    assert rc == case["proof_bytes"], rc
    return proofs, com, st


@pytest.mark.parametrize("shape", SMALL)
def test_proof_and_commitments_equal_the_golden_bytes(shape):
    case, coms, proofs, _ = agg_golden.load(shape)
    L = load_aggprove()
    draws = L.emul_aggprove_draws(case["k"], case["nd"])
    x, s, rnd = AP.batch(case, range(len(proofs)), draws)
    got, gcom, st = _prove(case, x, s, rnd)
    assert not st.any(), st.tolist()
    for b in range(len(proofs)):
        assert gcom[b].tobytes() == coms[b].tobytes(), (shape, b, "commitments")
        assert got[b].tobytes() == proofs[b].tobytes(), (shape, b, "proof")


def test_one_instance_of_the_sixteen_value_shape_equals_the_golden_bytes():
    shape = (16, 16, 16)
    case, coms, proofs, _ = agg_golden.load(shape)
    draws = load_aggprove().emul_aggprove_draws(16, 16)
    assert draws == 307
    x, s, rnd = AP.batch(case, [2], draws)
    got, gcom, st = _prove(case, x, s, rnd)
    assert not st.any()
    assert gcom[0].tobytes() == coms[2].tobytes() and got[0].tobytes() == proofs[2].tobytes()


def _rand_sc(*tag):
    return int.from_bytes(hashlib.shake_256(repr(tag).encode()).digest(40), "big") % A.N


@pytest.mark.parametrize("shape", SMALL)
def test_closed_form_collect_equals_the_pattern_walk(shape):
    k, nd, np_ = shape
    L = load_aggprove()
    nv, nm = nd + 1, k * nd
    words = (k * nv + nm + 3 * nm + 3 * nv) * 8
    for trial in range(2):
        lam, mu, e = (_rand_sc("collect", shape, trial, name) for name in ("lambda", "mu", "e"))
        walk, closed = np.full(words, 0xAAAAAAAA, np.uint32), np.full(words, 0x55555555, np.uint32)
        rc = L.emul_aggprove_collect(k, nd, np_, AP.be32(lam), AP.be32(mu), AP.be32(e), walk.ctypes.data, closed.ctypes.data)
        assert rc == words, rc
        wrong = np.flatnonzero(walk != closed)
        assert wrong.size == 0, (shape, trial, "first differing entry", int(wrong[0]) // 8)
        # two entries by hand, so that an error common to both sides would show: lambda_vec[1] = lambda, mu_vec[0] = mu
        limbs = lambda v: [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
        assert closed[8:16].tolist() == limbs(lam) and closed[k * nv * 8:k * nv * 8 + 8].tolist() == limbs(mu)
        # c_nR[0] = (S - lambda) / mu + e with S = sum over all (i, d) of lambda^(i nv + 1 + d)
        S = sum(pow(lam, i * nv + 1 + d, A.N) for i in range(k) for d in range(nd)) % A.N
        o = (k * nv + nm + nm) * 8
        assert closed[o:o + 8].tolist() == limbs(((S - lam) * pow(mu, -1, A.N) + e) % A.N)


def _witness(shape, xs, ss):
    k, nd, np_ = shape
    L = load_aggprove()
    n = len(xs)
    x = np.frombuffer(b"".join(AP.be32(v) for row in xs for v in row), np.uint8).copy()
    s = np.frombuffer(b"".join(AP.be32(v) for row in ss for v in row), np.uint8).copy()
    dig, m = np.full((n, k * nd, 32), 0xEE, np.uint8), np.full((n, np_, 32), 0xEE, np.uint8)
    st, rst, sc = np.full(n, 7, np.int32), np.full(n * k, 7, np.int32), np.full((n * k, 2, 32), 0xEE, np.uint8)
    assert L.emul_aggprove_witness(k, nd, np_, n, x.ctypes.data, s.ctypes.data, dig.ctypes.data, m.ctypes.data, st.ctypes.data, rst.ctypes.data,
                                   sc.ctypes.data) == 0
    val = lambda row: int.from_bytes(row.tobytes(), "big")
    return ([[val(r) for r in inst] for inst in dig], [[val(r) for r in inst] for inst in m], st, rst.reshape(n, k),
            [[(val(r[0]), val(r[1])) for r in sc[i * k:(i + 1) * k]] for i in range(n)])


def _expect(shape, xs):
    k, nd, np_ = shape
    flat = [d for x in xs for d in AP.digits_and_counts(x % (1 << 256), nd, np_)[0]]
    return flat, [flat.count(v) for v in range(np_)]


@pytest.mark.parametrize("shape", [(2, 4, 4), (3, 5, 10), (6, 2, 3), (2, 16, 16)])
def test_witness_digits_multiplicities_and_flags(shape):
    k, nd, np_ = shape
    top = np_**nd
    n = A.N
    rows = [
        ([0] * k, 0),                                                  # the low end of the range
        ([top - 1] * k, 0),                                            # the high end: every digit np - 1
        ([top - 1] * (k - 1) + [top], ST_OUT_OF_RANGE),                # one value one above the range
        ([1] + [n - 1] * (k - 1), ST_OUT_OF_RANGE),                    # n - 1: canonical, out of range
        ([n] + [3] * (k - 1), ST_BAD_ENCODING),                        # n: not canonical -- and nothing else
        ([n + 5] + [top] * (k - 1), ST_BAD_ENCODING | ST_OUT_OF_RANGE),    # a non-canonical and a canonical out-of-range value together
        ([_rand_sc("wit", shape, i) % top for i in range(k)], 0),
    ]
    xs = [r[0] for r in rows]
    ss = [[_rand_sc("s", shape, b, i) for i in range(k)] for b in range(len(rows))]
    dig, m, st, rst, sc = _witness(shape, xs, ss)
    for b, (x, want) in enumerate(rows):
        assert st[b] == want and (rst[b] == want).all(), (shape, b, st[b], want)
        canonical = [v % n if v < n else None for v in x]
        if all(v is not None for v in canonical):                      # (a non-canonical x has no agreed digits; the instance is flagged)
            d, mm = _expect(shape, x)
            assert dig[b] == d and m[b] == mm and sum(m[b]) == k * nd, (shape, b)
        if want == 0:
            assert sc[b] == [(x[i], ss[b][i]) for i in range(k)]
        else:
            assert sc[b] == [(0, 0)] * k                               # a flagged instance commits to zero scalars: identity points
    # a non-canonical s flags the instance like a non-canonical x
    dig, m, st, rst, sc = _witness(shape, [[1] * k, [2] * k], [[5] * (k - 1) + [n], [6] * k])
    assert st.tolist() == [ST_BAD_ENCODING, 0] and sc[0] == [(0, 0)] * k and sc[1] == [(2, 6)] * k


def test_one_bad_value_in_the_middle_flags_its_instance_alone():
    shape = (3, 4, 4)
    xs = [[5, 4**4, 7], [9, 10, 11]]
    ss = [[1, 2, 3], [4, 5, 6]]
    dig, m, st, rst, sc = _witness(shape, xs, ss)
    assert st.tolist() == [ST_OUT_OF_RANGE, 0]
    assert rst.tolist() == [[ST_OUT_OF_RANGE] * 3, [0] * 3]
    assert sc[0] == [(0, 0)] * 3 and sc[1] == [(9, 4), (10, 5), (11, 6)]
    d, mm = _expect(shape, xs[1])
    assert dig[1] == d and m[1] == mm
    # the flagged instance still has valid digits everywhere: the low four of 4^4 are zeros
    assert dig[0] == _expect(shape, [5, 0, 7])[0]


def test_a_flagged_instance_gets_zero_bytes_and_its_neighbour_the_golden_bytes():
    shape = (3, 4, 4)
    case, coms, proofs, _ = agg_golden.load(shape)
    draws = load_aggprove().emul_aggprove_draws(3, 4)
    x, s, rnd = AP.batch(case, [2, 2, 3], draws)
    x[0, 1] = np.frombuffer(AP.be32(4**4), np.uint8)                   # the middle value of instance 0
    got, gcom, st = _prove(case, x, s, rnd)
    assert st.tolist() == [ST_OUT_OF_RANGE, 0, 0]
    assert not got[0].any() and not gcom[0].any()
    assert got[1].tobytes() == proofs[2].tobytes() and gcom[1].tobytes() == coms[2].tobytes()
    assert got[2].tobytes() == proofs[3].tobytes() and gcom[2].tobytes() == coms[3].tobytes()


def test_argument_rules_on_a_grid():
    L = load_aggprove()
    for k in (0, 1, 2, 16, 64, 65):
        for nd in (0, 1, 4, 16, 63, 64):
            assert L.emul_aggprove_draws(k, nd) == k + 18 + (nd + 1) + k * nd
    for ng, nh in ((256, 32), (16, 16), (4096, 128)):
        for k in (0, 1, 2, 16, 64, 65):
            for nd in (0, 1, 2, 4, 16, 22, 23, 63, 64, 118):
                for np_ in (0, 1, 2, 3, 4, 16, 17, 18, 64, 65):
                    verifier = 1 <= k <= 64 and nd >= 1 and np_ >= 1 and k * nd <= ng and nd + 10 <= nh and np_ <= nd + 1
                    values = nd >= 1 and np_ >= 1 and (np_ == 1 or np_**nd <= A.N)
                    assert bool(L.emul_values_shape_ok(nd, np_)) == values, (nd, np_)
                    assert bool(L.emul_aggprove_shape_ok(k, nd, np_, ng, nh)) == (verifier and values), (k, nd, np_, ng, nh)
    # the shapes of the tests pass, the widths x does not determine are refused
    for shape in A.SHAPES:
        assert L.emul_aggprove_shape_ok(*shape, 256, 32)
    assert not L.emul_aggprove_shape_ok(2, 64, 16, 4096, 128) and L.emul_aggprove_shape_ok(2, 63, 16, 4096, 128)


def test_new_symbols_are_declared_and_bound():
    import os
    import re
    from bp_pp_amd import _capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "bppp.h")).read()
    ffi = open(os.path.join(root, "facade", "src", "ffi.rs")).read()
    names = ["bppp_reciprocal_agg_prove_draws", "bppp_reciprocal_agg_prove_values_batch", "bppp_reciprocal_agg_prove_values_batch_seeded",
             "bppp_reciprocal_agg_prove_values_batch_device", "bppp_reciprocal_agg_prove_values_batch_seeded_device"]
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, ffi), name
        assert name in _capi.EXPORTS
