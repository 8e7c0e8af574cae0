"""CPU tier for the mixed-value-count aggregate PROVER's device code (bp_pp_amd/csrc/agg_prove_mixed_core.h and the generic circuit /
WNLA prover stages behind it, compiled for the host: tests/emul/aggprove_mixed_emul.cpp), one "thread" after the other in the order
agg_prove_mixed_part launches the kernels.  Every comparison is bit-exact.

  * golden bytes for every count: on the three small context shapes ks cycles through all counts, unused x, s and rnd slots hold 0xFF
    and the workspace was last used by a call with k_max in every row; every row's commitments and proof are the golden pool's bytes
    (tests/golden/agg_mixed_cases.json) and everything behind them in both slots is zero;
  * the padding is zero: the scalar sets of c_o, c_l, c_r and c_s and the WNLA witness n behind k_t nd, the value and pole rows i >= k_t;
  * with all ks equal the outputs are the uniform emulation's (tests/emul/aggprove_emul.cpp), for k = k_max and for a k < k_max;
  * a count of 0 or k_max + 1 is flagged and zeroed, and its neighbours' outputs are those of the call without it."""
import numpy as np
import pytest

import agg_golden
import agg_mixed_cases as M
import agg_prove_mixed_cases as PM
from emul.build import load as load_emul
from emul.build_aggprove import load as load_aggprove
from emul.build_aggprove_mixed import load as load_mixed

W = 4
SMALL = [s for s in M.CONTEXTS if s != (16, 16, 16)]
ST_BAD_ENCODING = 1
_tables, _runs = {}, {}


def _table(case_max):
    key = (case_max["k"], case_max["nd"])
    if key not in _tables:
        L = load_emul()
        gens = agg_golden.generators(case_max)
        NB = 1 + case_max["NG"] + case_max["NH"]
        tab = np.zeros(L.emul_fb_table_entries(NB, W) * 64, dtype=np.uint8)
        assert L.emul_fb_build(gens, NB, W, tab.ctypes.data) == 0
        _tables[key] = tab
    return _tables[key]


def run(shape, ks, x, s, rnd, prev=None):
    """-> dict(proofs, com, st, msc_a [3, NB, 8, n], msc_b [NB, 8, n], wn_n [n, NG, 32], vsc [2, 8, n k], rsc [nv, 8, n k])"""
    L = load_mixed()
    case_max, _ = M.load_pool(shape)
    k, nd, np_ = shape
    NG, NH = case_max["NG"], case_max["NH"]
    n, NB = len(ks), 1 + NG + NH
    ks = np.ascontiguousarray(ks, np.uint8)
    x, s, rnd = (np.ascontiguousarray(a) for a in (x, s, rnd))
    assert x.shape == s.shape == (n, k, 32) and rnd.shape == (n, PM.draws(k, nd), 32)
    out = dict(proofs=np.full((n, case_max["proof_bytes"]), 0xEE, np.uint8), com=np.full((n, k, 64), 0xEE, np.uint8), st=np.full(n, 7, np.int32),
               msc_a=np.full((3, NB, 8, n), 0xEE, np.uint32), msc_b=np.full((NB, 8, n), 0xEE, np.uint32), wn_n=np.full((n, NG, 32), 0xEE, np.uint8),
               vsc=np.full((2, 8, n * k), 0xEE, np.uint32), rsc=np.full((nd + 1, 8, n * k), 0xEE, np.uint32))
    pv = [None] * 4 if prev is None else [np.ascontiguousarray(a) for a in prev]
    tab = _table(case_max)
    rc = L.emul_aggprove_mixed(tab.ctypes.data, W, NG, NH, k, nd, np_, case_max["label"], len(case_max["label"]), n, ks.ctypes.data,
                               x.ctypes.data, s.ctypes.data, rnd.ctypes.data, *[None if a is None else a.ctypes.data for a in pv],
                               out["proofs"].ctypes.data, out["com"].ctypes.data, out["st"].ctypes.data, out["msc_a"].ctypes.data,
                               out["msc_b"].ctypes.data, out["wn_n"].ctypes.data, out["vsc"].ctypes.data, out["rsc"].ctypes.data)
    assert rc == case_max["proof_bytes"], rc
    return out


def _cycled(shape):
    """Every count twice and one more row, neighbours differing, behind a call of k_max in every row on the same workspace."""
    if shape not in _runs:
        ks = PM.cycle(shape, 2 * len(M.CONTEXTS[shape]) + 1)
        x, s, rnd, C, Q = PM.build(shape, ks)
        px, ps, prnd, _, _ = PM.build(shape, [shape[0]] * len(ks))
        prev = (np.full(len(ks), shape[0], np.uint8), px, ps, prnd)
        _runs[shape] = (ks, C, Q, run(shape, ks, x, s, rnd, prev=prev))
    return _runs[shape]


@pytest.mark.parametrize("shape", SMALL)
def test_every_count_gives_the_golden_bytes_and_zeros_behind_them(shape):
    ks, C, Q, out = _cycled(shape)
    assert sorted(set(ks)) == M.CONTEXTS[shape] and all(a != b for a, b in zip(ks, ks[1:]))
    assert not out["st"].any(), out["st"].tolist()
    case_max, _ = M.load_pool(shape)
    for t, k in enumerate(ks):
        pb = M.setup_on(case_max, k)["proof_bytes"]
        assert Q[t, :pb].any() and not Q[t, pb:].any()                     # (the expectation itself: the pool's bytes, zero-extended)
        assert out["com"][t].tobytes() == C[t].tobytes(), (shape, t, k, "commitments")
        assert out["proofs"][t].tobytes() == Q[t].tobytes(), (shape, t, k, "proof")


@pytest.mark.parametrize("shape", SMALL)
def test_padding_is_zero(shape):
    ks, _, _, out = _cycled(shape)
    k_max, nd, _ = shape
    case_max, _ = M.load_pool(shape)
    NG = case_max["NG"]
    for t, k in enumerate(ks):
        nm = k * nd
        # slot = base index: g_vec[j] is base 1 + j.  The reciprocals (c_r's set) are never zero: the entries in front of the padding are there
        assert out["msc_a"][2, 1:1 + nm, :, t].any(axis=1).all(), (shape, t)
        for name, sets in (("c_o", out["msc_a"][0]), ("c_l", out["msc_a"][1]), ("c_r", out["msc_a"][2]), ("c_s", out["msc_b"])):
            assert not sets[1 + nm:1 + NG, :, t].any(), (shape, t, k, name)
        assert out["wn_n"][t, :nm].any() and not out["wn_n"][t, nm:].any(), (shape, t, k, "wn_n")
        rows = slice(t * k_max + k, (t + 1) * k_max)
        assert not out["vsc"][:, :, rows].any() and not out["rsc"][:, :, rows].any(), (shape, t, k, "rows")
        used = slice(t * k_max, t * k_max + k)
        assert out["rsc"][:, :, used].any(axis=1).all()                    # rb_i and every reciprocal of a used row


def _uniform(shape, k, x, s, rnd):
    L = load_aggprove()
    case_max, _ = M.load_pool(shape)
    case = M.setup_on(case_max, k)
    n = x.shape[0]
    x, s, rnd = (np.ascontiguousarray(a) for a in (x, s, rnd))
    proofs, com, st = np.full((n, case["proof_bytes"]), 0xEE, np.uint8), np.full((n, k, 64), 0xEE, np.uint8), np.full(n, 7, np.int32)
    tab = _table(case_max)
    rc = L.emul_aggprove(tab.ctypes.data, W, case_max["NG"], case_max["NH"], k, shape[1], shape[2], case_max["label"], len(case_max["label"]), n,
                         x.ctypes.data, s.ctypes.data, rnd.ctypes.data, proofs.ctypes.data, com.ctypes.data, st.ctypes.data)
    assert rc == case["proof_bytes"], rc
    return proofs, com, st


@pytest.mark.parametrize("shape,k", [((3, 4, 4), 3), ((3, 4, 4), 2), ((7, 3, 4), 7), ((7, 3, 4), 4), ((6, 2, 3), 1)])
def test_equal_counts_give_the_uniform_path_s_outputs(shape, k):
    n = 3
    x, s, rnd, _, _ = PM.build(shape, [k] * n)
    out = run(shape, [k] * n, x, s, rnd)
    D = PM.draws(k, shape[1])
    up, uc, ust = _uniform(shape, k, x[:, :k], s[:, :k], rnd[:, :D])
    pb = up.shape[1]
    assert out["st"].tobytes() == ust.tobytes() and not ust.any()
    assert out["proofs"][:, :pb].tobytes() == up.tobytes() and not out["proofs"][:, pb:].any()
    assert out["com"][:, :k].tobytes() == uc.tobytes() and not out["com"][:, k:].any()


@pytest.mark.parametrize("shape", [(3, 4, 4), (7, 3, 4)])
def test_a_bad_count_is_flagged_and_touches_nothing_else(shape):
    k_max = shape[0]
    ks = PM.cycle(shape, 7, start=1)
    x, s, rnd, C, Q = PM.build(shape, ks)
    clean = run(shape, ks, x, s, rnd)
    assert not clean["st"].any() and clean["proofs"].tobytes() == Q.tobytes() and clean["com"].tobytes() == C.tobytes()
    bad = {0: 0, 3: k_max + 1, 6: 255}
    ks2 = list(ks)
    x2, s2 = x.copy(), s.copy()
    for t, k in bad.items():
        ks2[t] = k
        x2[t], s2[t] = 0xFF, 0xFF                                         # (nothing of a bad instance's x or s is read)
    out = run(shape, ks2, x2, s2, rnd)
    assert out["st"].tolist() == [ST_BAD_ENCODING if t in bad else 0 for t in range(len(ks))]
    for t in range(len(ks)):
        if t in bad:
            assert not out["proofs"][t].any() and not out["com"][t].any(), t
        else:
            assert out["proofs"][t].tobytes() == clean["proofs"][t].tobytes() and out["com"][t].tobytes() == clean["com"][t].tobytes(), t


def test_a_flagged_value_zeroes_its_instance_alone():
    shape = (3, 4, 4)
    ks = [3, 1, 2, 3]
    x, s, rnd, C, Q = PM.build(shape, ks)
    x, s = x.copy(), s.copy()
    x[2, 1] = np.frombuffer((4**4).to_bytes(32, "big"), np.uint8)          # the last USED value of row 2 one above the range
    out = run(shape, ks, x, s, rnd)
    assert out["st"].tolist() == [0, 0, 4, 0]
    for t in (0, 1, 3):
        assert out["proofs"][t].tobytes() == Q[t].tobytes() and out["com"][t].tobytes() == C[t].tobytes(), t
    assert not out["proofs"][2].any() and not out["com"][2].any()


def test_the_argument_rule():
    L = load_mixed()
    arr = lambda v: np.asarray(v, np.uint8)

    def ok(k_max, nd, np_, ks, dev=0, n=None, ng=256, nh=32):
        a = None if ks is None else arr(ks)
        return bool(L.emul_aggprove_mixed_args_ok(ng, nh, len(ks) if n is None else n, k_max, None if a is None else a.ctypes.data, dev, nd, np_))

    assert ok(16, 16, 16, [1, 16, 9]) and ok(16, 16, 16, [1, 16, 9], dev=1)
    assert not ok(16, 16, 16, None, n=0) and not ok(16, 16, 16, None, dev=1, n=2)
    assert not ok(16, 16, 16, [0, 1]) and not ok(16, 16, 16, [1, 17]) and ok(16, 16, 16, [0, 17], dev=1) and ok(16, 16, 16, [0, 17], n=0)
    assert not ok(0, 16, 16, [1]) and not ok(65, 1, 1, [1]) and not ok(16, 17, 16, [1]) and not ok(2, 23, 16, [1]) and not ok(16, 16, 18, [1])
    assert ok(1, 16, 16, [1]) and not ok(1, 16, 16, [2])
