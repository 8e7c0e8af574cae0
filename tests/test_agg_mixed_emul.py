"""CPU tier for the mixed-value-count aggregate verifier's device code (bp_pp_amd/csrc/agg_mixed_core.h compiled for the host,
tests/emul/agg_mixed_emul.cpp), on the fixture of tests/agg_mixed_cases.py:

  * the verdict and the status of every row of the batch are the oracle's (golden file), one lane and as G = 2, 4, 8 runs, on the
    affine-table and the projective-table form of C0's variable-base half;
  * on clean rows of every value count the trace is the oracle's: e, the sums V_i + R_i, rho, mu, c, ps_tau, pn_tau, C0;
  * every word of sc0 behind an instance's k_i nd entries of pn_tau, its coefficient slots and its point slots behind k_i are zero --
    after a call on the same workspace in which the row had k_max values;
  * the fixed-base sum forms (lanes 1, 8, 64 walked serially, as the kernels' lanes) on those padded scalar sets, with zeros at the
    end, in the middle and for a whole instance, give the oracle's sum;
  * with all ks equal the mixed path's sc0, pts, wn_c and wn_commit are the uniform path's word for word."""
import numpy as np
import pytest

import agg_cases as A
import agg_golden
import agg_mixed_cases as M
import bppp_oracle as O
from emul.build import load as load_emul
from emul.build_agg_mixed import load as load_mixed

W = 4
SMALL = [s for s in M.CONTEXTS if s != (16, 16, 16)]
_tables = {}


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


def run(case_max, ks, C, Q, G=1, slow=0, nl_fixed=8, prev_ks=None):
    L = load_mixed()
    k, nd, NH = case_max["k"], case_max["nd"], case_max["NH"]
    n = len(ks)
    ks, C, Q = np.ascontiguousarray(ks, np.uint8), np.ascontiguousarray(C), np.ascontiguousarray(Q)
    assert C.shape == (n, k, 64) and Q.shape == (n, case_max["proof_bytes"])
    lnb = 32 * (case_max["nl"] + case_max["nn"])
    out = dict(rho=np.zeros((n, 32), np.uint8), mu=np.zeros((n, 32), np.uint8), c=np.zeros((n, NH, 32), np.uint8),
               c0=np.zeros((n, 64), np.uint8), p1=np.zeros(n, np.int32), acc=np.zeros(n, np.uint8), st=np.zeros(n, np.int32),
               sc0=np.zeros((k * nd + 5 + k, 8, n), np.uint32), pts=np.zeros((4 + k, 16, n), np.uint32), ln=np.zeros((n, lnb), np.uint8),
               einv=np.zeros((8, n), np.uint32))
    prev = None if prev_ks is None else np.ascontiguousarray(prev_ks, np.uint8)
    tab = _table(case_max)
    rc = L.emul_agg_mixed_verify(tab.ctypes.data, W, case_max["NG"], NH, k, nd, case_max["np"], case_max["label"], len(case_max["label"]), n,
                                 ks.ctypes.data, None if prev is None else prev.ctypes.data, C.ctypes.data, Q.ctypes.data, case_max["rounds"],
                                 case_max["nl"], case_max["nn"], G, slow, nl_fixed, out["rho"].ctypes.data, out["mu"].ctypes.data,
                                 out["c"].ctypes.data, out["c0"].ctypes.data, out["p1"].ctypes.data, out["acc"].ctypes.data,
                                 out["st"].ctypes.data, out["sc0"].ctypes.data, out["pts"].ctypes.data, out["ln"].ctypes.data,
                                 out["einv"].ctypes.data)
    assert rc == 0
    return out


def run_uniform(case_max, case, C, Q, G=1, slow=0):
    """The uniform path on dense inputs of case["k"] values (generators: the context's, which the case shares)."""
    L = load_mixed()
    k, nd, NH = case["k"], case["nd"], case["NH"]
    n = C.shape[0]
    C, Q = np.ascontiguousarray(C), np.ascontiguousarray(Q)
    assert C.shape == (n, k, 64) and Q.shape == (n, case["proof_bytes"])
    out = dict(c=np.zeros((n, NH, 32), np.uint8), c0=np.zeros((n, 64), np.uint8), st=np.zeros(n, np.int32),
               sc0=np.zeros((k * nd + 5 + k, 8, n), np.uint32), pts=np.zeros((4 + k, 16, n), np.uint32))
    tab = _table(case_max)
    rc = L.emul_agg_uniform_c0(tab.ctypes.data, W, case["NG"], NH, k, nd, case["np"], case["label"], len(case["label"]), n, C.ctypes.data,
                               Q.ctypes.data, case["rounds"], case["nl"], case["nn"], G, slow, out["c"].ctypes.data, out["c0"].ctypes.data,
                               out["st"].ctypes.data, out["sc0"].ctypes.data, out["pts"].ctypes.data)
    assert rc == 0
    return out


def _be(row):
    return int.from_bytes(row.tobytes(), "big")


def _words(w):
    """A workspace value: 8 little-endian 32-bit words."""
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def _point(pts, slot, t):
    x, y = _words(pts[slot, :8, t]), _words(pts[slot, 8:, t])
    return x.to_bytes(32, "big") + y.to_bytes(32, "big")


def _assert_trace(case_max, out, ks, C, Q, row):
    case, com, proof = M.row_inputs(case_max, ks, C, Q, row)
    k, nd = case["k"], case["nd"]
    tr = []
    assert A.verify(case, com, proof, tr) == 1
    d = {key: v for key, v in tr if not key.startswith("wnla")}
    assert _words(out["einv"][:, row]) == O.sc_inv(d["e"])
    assert [_point(out["pts"], 4 + i, row) for i in range(k)] == [O.pt_to_xy64(p) for p in d["V+R"]]
    assert _be(out["rho"][row]) == d["rho"] and _be(out["mu"][row]) == d["rho"] * d["rho"] % O.N
    assert [_be(r) for r in out["c"][row]] == d["c"]
    assert _words(out["sc0"][0, :, row]) == d["ps_tau"]
    assert [_words(out["sc0"][1 + j, :, row]) for j in range(k * nd)] == d["pn_tau"]
    assert out["c0"][row].tobytes() == O.pt_to_xy64(d["C0"])
    assert out["p1"][row] == 0 and out["acc"][row] == 1 and out["st"][row] == 0
    assert out["ln"][row].tobytes() == proof[-out["ln"].shape[1]:]


def _assert_padding_is_zero(case_max, out, ks):
    k_max, nd = case_max["k"], case_max["nd"]
    nm = k_max * nd
    for t, k in enumerate(np.asarray(ks).tolist()):
        k = k if 1 <= k <= k_max else 1
        assert not out["sc0"][1 + k * nd:1 + nm, :, t].any(), ("pn_tau padding", t, k)
        assert not out["sc0"][5 + nm + k:, :, t].any(), ("coefficient padding", t, k)
        assert not out["pts"][4 + k:, :, t].any(), ("point padding", t, k)
        assert out["sc0"][1:1 + k * nd, :, t].any(axis=1).all() and out["sc0"][1 + nm:5 + nm + k, :, t].any(axis=1).all()


@pytest.mark.parametrize("shape", SMALL)
def test_every_row_gets_the_oracle_verdict_on_both_c0_paths_after_a_larger_call(shape):
    """The whole batch: clean rows of every value count next to each other, every corrupted field class on the smallest and the
    largest count, unused slot bytes of 0xFF and of another proof, a proof under a wrong count.  The workspace held a call with
    k_max values in every row before (prev_ks): what phase 1 leaves behind k_i is zero all the same."""
    case_max, ks, C, Q, acc, flag, notes = M.batch(shape)
    prev = np.full(M.ROWS, shape[0], np.uint8)
    for slow in (0, 1):
        o = run(case_max, ks, C, Q, slow=slow, prev_ks=prev)
        wrong = [(r, dict(notes).get(r, "clean"), int(o["acc"][r]), int(o["st"][r])) for r in range(M.ROWS) if o["acc"][r] != acc[r]]
        assert not wrong, (shape, slow, wrong)
        assert ((o["st"] != 0) == flag).all() and ((o["st"] & 1 != 0) == flag).all(), (shape, slow, o["st"].tolist())
        _assert_padding_is_zero(case_max, o, ks)
    noted = dict(notes)
    for r in range(M.ROWS):
        if noted.get(r) in ("unused_ff", "unused_other"):
            assert acc[r] == 1 and not flag[r]


@pytest.mark.parametrize("shape", SMALL)
def test_clean_rows_of_every_value_count_equal_the_oracle_trace(shape):
    case_max, ks, C, Q, _, _, notes = M.batch(shape)
    rows = list(range(len(M.CONTEXTS[shape]))) + [r for r, what in notes if what.startswith("unused")]
    o = run(case_max, ks, C, Q)
    for r in rows:
        _assert_trace(case_max, o, ks, C, Q, r)


@pytest.mark.parametrize("shape", SMALL)
def test_lane_group_runs_sum_to_the_one_lane_result(shape):
    """G = 2, 4, 8: the runs over k_i nd entries (1 .. 21 entries against up to 8 runs: empty runs, runs across value boundaries) and
    the padding's pieces; every output byte is the one-lane form's, on clean and on corrupted rows, after a larger call."""
    case_max, ks, C, Q, _, _, _ = M.batch(shape)
    sel = np.r_[0:len(M.CONTEXTS[shape]) + 3, M.CLEAN:M.CLEAN + 8, M.ROWS - 5:M.ROWS]
    ks, C, Q = ks[sel], C[sel], Q[sel]
    prev = np.full(len(sel), shape[0], np.uint8)
    ref = run(case_max, ks, C, Q)
    for G in (2, 4, 8):
        o = run(case_max, ks, C, Q, G=G, prev_ks=prev)
        for key in ref:
            assert (o[key] == ref[key]).all(), (shape, G, key)


def test_the_16_value_context_equals_the_oracle_trace_in_every_form():
    """(16, 16, 16) with k_i = 1, 9, 15, 16: one oracle proof each; runs of 128 / 64 / 32 entries against k_i nd = 16, 144, 240, 256."""
    shape = (16, 16, 16)
    case_max, ks, C, Q, acc, flag, _ = M.batch(shape)
    assert (case_max["NG"], case_max["NH"], case_max["rounds"], case_max["nl"], case_max["nn"], case_max["proof_bytes"]) == (256, 32, 6, 1, 4, 2208)
    ks, C, Q = ks[:4], C[:4], Q[:4]
    assert ks.tolist() == [1, 9, 15, 16]
    prev = np.full(4, 16, np.uint8)
    ref = run(case_max, ks, C, Q, prev_ks=prev)
    assert ref["acc"].tolist() == [1, 1, 1, 1] and not ref["st"].any()
    _assert_padding_is_zero(case_max, ref, ks)
    for r in (0, 1, 2):
        _assert_trace(case_max, ref, ks, C, Q, r)
    for G in (2, 4, 8):
        o = run(case_max, ks, C, Q, G=G, prev_ks=prev)
        assert all((o[key] == ref[key]).all() for key in ref), G


def _oracle_sum(case_max, scalars):
    """sum_j scalars[j] * base_j over g | g_vec || g_vec_ -> 64 bytes (the identity: zeros)."""
    bases = [case_max["Pg"]] + case_max["Pgv"] + case_max["Pgv_"]
    terms = [(s, b) for s, b in zip(scalars, bases) if s]
    if not terms:
        return bytes(64)
    return O.pt_to_xy64(O.vector_mul([b for _, b in terms], [s for s, _ in terms], O.PT))


@pytest.mark.parametrize("shape", [(3, 4, 4), (7, 3, 4)])
def test_fixed_base_sum_forms_on_zero_padded_scalars_equal_the_oracle_sum(shape):
    """ps_tau | pn_tau[k_i nd] | zeros up to k_max nd as phase 1 leaves them -- zeros at the END --, the same with entries in the MIDDLE
    zeroed, and a WHOLE instance of zeros, next to each other: the sum over the uniform range 1 + k_max nd in the serial order of 1, 8
    and 64 lanes per instance is the oracle's sum of the non-zero terms."""
    case_max, ks, C, Q, _, _, _ = M.batch(shape)
    n0 = len(M.CONTEXTS[shape])
    o = run(case_max, ks[:n0], C[:n0], Q[:n0])
    count = 1 + case_max["k"] * case_max["nd"]
    sets = [o["sc0"][:count, :, t].copy() for t in range(n0)]
    mid = sets[-1].copy()
    mid[2:count - 2:2] = 0                          # every other entry of the largest instance
    hole = sets[n0 // 2].copy()
    hole[0] = 0                                     # no ps_tau term: the sum starts at a later base
    sets += [mid, hole, np.zeros_like(mid)]
    sc0 = np.ascontiguousarray(np.stack(sets, axis=2))
    n = sc0.shape[2]
    expect = [_oracle_sum(case_max, [_words(sc0[j, :, t]) for j in range(count)]) for t in range(n)]
    assert expect[-1] == bytes(64) and len(set(expect)) == n
    L = load_mixed()
    tab = _table(case_max)
    for nl in (1, 8, 64):
        out = np.zeros((n, 64), np.uint8)
        assert L.emul_agg_mixed_fixed_sum(tab.ctypes.data, W, n, count, sc0.ctypes.data, nl, out.ctypes.data) == 0
        assert [out[t].tobytes() for t in range(n)] == expect, nl


@pytest.mark.parametrize("shape,k", [((3, 4, 4), 3), ((3, 4, 4), 1), ((7, 3, 4), 7), ((7, 3, 4), 4), ((6, 2, 3), 6), ((16, 16, 16), 16)])
def test_all_equal_ks_is_the_uniform_path_word_for_word(shape, k):
    """Rows of one value count, clean and corrupted: with k = k_max the two workspaces have one layout and every word of sc0 and pts,
    wn_c and wn_commit is equal; with k < k_max the uniform path's entries sit where the k_max layout puts them."""
    case, ks, C, Q, _, _ = M.uniform_batch(shape, k)
    case_max = M.load_pool(shape)[0]
    n = min(len(ks), 3 if shape == (16, 16, 16) else 12)
    ks, C, Q = ks[:n], C[:n], Q[:n]
    Cd, Qd = np.ascontiguousarray(C[:, :k]), np.ascontiguousarray(Q[:, :case["proof_bytes"]])
    for G in (1, 4):
        m, u = run(case_max, ks, C, Q, G=G), run_uniform(case_max, case, Cd, Qd, G=G)
        assert m["c"].tobytes() == u["c"].tobytes() and m["c0"].tobytes() == u["c0"].tobytes(), (shape, k, G)
        assert (m["p1"] == u["st"]).all()
        if k == shape[0]:
            assert m["sc0"].tobytes() == u["sc0"].tobytes() and m["pts"].tobytes() == u["pts"].tobytes()
        else:
            nm, nm_max = k * shape[1], shape[0] * shape[1]
            assert (m["sc0"][:1 + nm] == u["sc0"][:1 + nm]).all() and (m["sc0"][1 + nm_max:5 + nm_max + k] == u["sc0"][1 + nm:]).all()
            assert (m["pts"][:4 + k] == u["pts"]).all()


def test_a_count_outside_the_range_is_flagged_and_touches_no_other_instance():
    """What the device form meets when d_ks holds a 0 or k_max + 1: the instance is flagged BPPP_ST_BAD_ENCODING in phase 1, rejected,
    and runs on harmless values; its neighbours' outputs are those of the call without it."""
    shape = (3, 4, 4)
    case_max, ks, C, Q, acc, _, _ = M.batch(shape)
    ks, C, Q = ks[:9].copy(), C[:9], Q[:9]
    ref = run(case_max, ks, C, Q)
    bad = ks.copy()
    bad[2], bad[5] = 0, shape[0] + 1
    for G in (1, 2):
        o = run(case_max, bad, C, Q, G=G)
        assert o["acc"][[2, 5]].tolist() == [0, 0] and (o["st"][[2, 5]] & 1).tolist() == [1, 1] and (o["p1"][[2, 5]] & 1).tolist() == [1, 1]
        keep = [i for i in range(9) if i not in (2, 5)]
        for key in ("rho", "mu", "c", "c0", "acc", "st", "ln"):
            assert (o[key][keep] == ref[key][keep]).all(), key
        assert (o["sc0"][:, :, keep] == ref["sc0"][:, :, keep]).all() and (o["pts"][:, :, keep] == ref["pts"][:, :, keep]).all()
        assert not o["pts"][:, :, [2, 5]].any()      # identity points everywhere
