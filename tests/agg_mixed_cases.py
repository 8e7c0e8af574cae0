"""Aggregated reciprocal range proofs of MIXED value counts on one context (bppp_reciprocal_agg_verify_batch_mixed): the oracle cases,
the golden pool (tests/golden/agg_mixed_cases.json, written by tests/golden/make_agg_mixed_cases.py with the in-repo oracle only) and
the test batch.

A context shape (k_max, nd, np) is agg_cases.setup(k_max, nd, np).  setup_on(case_max, k) is the oracle case of a proof over k values
on THAT context's generators: g_vec || g_vec_ is one vector of NG points, of which the first k nd are the case's g_vec and the rest
its padding; h_vec, h_vec_, NG, NH and so (rounds, nl, nn) are the context's.  (tests/golden/agg_cases.json's proofs for smaller k sit
on other padding generators and are of no use here.)

The batch, ROWS rows in slots laid out by k_max (commitments [ROWS, k_max, 64], proofs [ROWS, proof_bytes(k_max)], zero behind what
an instance uses unless a row says otherwise):
    rows 0 .. CLEAN-1        clean; ks cycles through the shape's value counts, so neighbouring lanes of a wavefront differ
    then two rows per KIND   one field class of agg_cases.corrupted_batch each, on the smallest and on the largest k_i
    unused_ff                the smallest k_i with every unused byte of both slots 0xFF
    unused_other             the smallest k_i in front of a valid k_max proof's bytes and commitments
    wrong_k_plus             a valid k_min proof under ks[i] = k_min + 1
    wrong_k_minus            a valid k_max proof under ks[i] = k_max - 1
    n_last_row               the last row: a scalar of n changed (what a short grid drops)
Expectations are the oracle's verify(setup_on(case_max, ks[i]), ...) on what the row's first ks[i] commitments and
proof_bytes(ks[i]) bytes hold, for EVERY row, recorded in the JSON."""
import json
import os

import numpy as np

import agg_cases as A

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_mixed_cases.json")
# context shape -> the value counts of its instances (why these: the table in tests/test_gpu_agg_mixed.py)
CONTEXTS = {(3, 4, 4): [1, 2, 3], (7, 3, 4): [1, 2, 3, 4, 5, 6, 7], (6, 2, 3): [1, 2, 3, 4, 5, 6], (16, 16, 16): [1, 9, 15, 16]}
POOL = {(16, 16, 16): 1}       # oracle proofs per value count (default 2)
CLEAN = 28
KINDS = ["c_l", "c_r", "c_o", "c_s", "r", "x", "R_first", "R_mid", "R_last", "l", "n", "V_first", "V_last", "V_swapped", "R_off_curve",
         "V_off_curve", "coordinate_p", "V_eq_R", "V_eq_negR"]
ROWS = CLEAN + 2 * len(KINDS) + 5
_cache = {}


def setup_on(case_max, k):
    """The oracle case for k values on the generators of case_max's context."""
    nd, NG = case_max["nd"], case_max["NG"]
    assert 1 <= k <= case_max["k"]
    allg, allP = case_max["gv"] + case_max["gv_"], case_max["Pgv"] + case_max["Pgv_"]
    case = dict(case_max)
    case.update(k=k, nm=k * nd, gv=allg[:k * nd], gv_=allg[k * nd:NG], Pgv=allP[:k * nd], Pgv_=allP[k * nd:NG])
    case["proof_bytes"] = A.proof_bytes(k, case["rounds"], case["nl"], case["nn"])
    return case


def pool_size(shape):
    return POOL.get(shape, 2)


def corrupt_row(case, c, q, kind, donor_v=None):
    """One field class of agg_cases.corrupted_batch on one row, in place: c [k, 64], q [proof_bytes(k)] (views into the slots)."""
    k, off = case["k"], A.field_offsets(case)
    neg = lambda xy: np.frombuffer(A.neg_point(xy.tobytes()), np.uint8)
    if kind in ("c_l", "c_r", "c_o", "c_s", "r", "x", "R_first", "R_mid", "R_last"):      # a valid but wrong point: another field's
        o, other = off[kind], off["c_s" if kind != "c_s" else "c_l"]
        q[o:o + 64] = q[other:other + 64].copy()
    elif kind in ("l", "n"):
        q[off[kind] + 31] ^= 1
    elif kind == "V_first":
        c[0] = donor_v if donor_v is not None else neg(c[0])
    elif kind == "V_last":
        c[k - 1] = neg(c[k - 1])
    elif kind == "V_swapped":
        if k > 1:
            c[[0, 1]] = c[[1, 0]]
        else:
            c[0] = neg(c[0])                      # (one value has nothing to swap: its V negated)
    elif kind == "R_off_curve":
        q[off["R_mid"] + 40] ^= 1
    elif kind == "V_off_curve":
        c[k - 1, 63] ^= 1
    elif kind == "coordinate_p":
        q[off["c_o"]:off["c_o"] + 32] = np.frombuffer(A.FIELD_P.to_bytes(32, "big"), np.uint8)
    elif kind == "V_eq_R":
        c[k - 1] = q[off["R_last"]:off["R_last"] + 64]
    elif kind == "V_eq_negR":
        c[0] = neg(q[off["R_first"]:off["R_first"] + 64])
    elif kind == "n_last_row":
        q[off["n"] + 30] ^= 4
    else:
        raise ValueError(kind)


def build_batch(shape, pool):
    """pool: {k: [(commitments bytes, proof bytes)]} -> (ks [ROWS], C [ROWS, k_max, 64], Q [ROWS, stride], notes [(row, what)]).
    Deterministic: the golden file's expectations are for exactly this batch."""
    k_max, KS = shape[0], CONTEXTS[shape]
    case_max = A.setup(*shape)
    kmin, kmax = KS[0], KS[-1]
    assert kmax == k_max and kmin + 1 <= k_max and kmax >= 2
    ks = np.zeros(ROWS, np.uint8)
    C = np.zeros((ROWS, k_max, 64), np.uint8)
    Q = np.zeros((ROWS, case_max["proof_bytes"]), np.uint8)
    notes = []

    def put(row, k, j, as_k=None):
        com, proof = pool[k][j % len(pool[k])]
        ks[row] = k if as_k is None else as_k
        C[row, :k] = np.frombuffer(com, np.uint8).reshape(k, 64)
        Q[row, :len(proof)] = np.frombuffer(proof, np.uint8)

    for row in range(CLEAN):
        put(row, KS[row % len(KS)], row // len(KS))
    row = CLEAN
    for j, kind in enumerate(KINDS):
        for k in (kmin, kmax):
            put(row, k, j)
            case = setup_on(case_max, k)
            donor = np.frombuffer(pool[k][(j + 1) % len(pool[k])][0], np.uint8)[:64] if len(pool[k]) > 1 else None
            corrupt_row(case, C[row, :k], Q[row, :case["proof_bytes"]], kind, donor)
            notes.append((row, "%s,k=%d" % (kind, k)))
            row += 1
    pb_min = A.proof_bytes(kmin, case_max["rounds"], case_max["nl"], case_max["nn"])
    C[row] = 0xFF; Q[row] = 0xFF
    put(row, kmin, 1)
    assert (C[row, kmin:] == 0xFF).all() and (Q[row, pb_min:] == 0xFF).all()
    notes.append((row, "unused_ff")); row += 1
    put(row, kmax, 0)
    put(row, kmin, 0)
    notes.append((row, "unused_other")); row += 1
    put(row, kmin, 0, as_k=kmin + 1)
    notes.append((row, "wrong_k_plus")); row += 1
    put(row, kmax, 0, as_k=kmax - 1)
    notes.append((row, "wrong_k_minus")); row += 1
    put(row, kmax, 1)
    case = setup_on(case_max, kmax)
    corrupt_row(case, C[row, :kmax], Q[row, :case["proof_bytes"]], "n_last_row")
    notes.append((row, "n_last_row")); row += 1
    assert row == ROWS
    return ks, C, Q, notes


def row_inputs(case_max, ks, C, Q, row):
    """What the verifier may read of a row: (case for ks[row], commitments bytes, proof bytes)."""
    case = setup_on(case_max, int(ks[row]))
    return case, C[row, :case["k"]].tobytes(), Q[row, :case["proof_bytes"]].tobytes()


def _file():
    if "file" not in _cache:
        with open(PATH) as f:
            _cache["file"] = json.load(f)
    return _cache["file"]


def load_pool(shape):
    """-> (case_max, {k: [(commitments bytes, proof bytes)]})"""
    key = ("pool", shape)
    if key not in _cache:
        g = _file()["%d,%d,%d" % shape]
        case_max = A.setup(*shape)
        assert (g["rounds"], g["nl"], g["nn"]) == (case_max["rounds"], case_max["nl"], case_max["nn"])
        _cache[key] = (case_max, {int(k): [(bytes.fromhex(c), bytes.fromhex(p)) for c, p in v] for k, v in g["pool"].items()})
    return _cache[key]


def batch(shape):
    """-> (case_max, ks, C, Q, expect_acc [ROWS], expect_flag [ROWS], notes): the batch and the oracle's verdict on every row."""
    key = ("batch", shape)
    if key not in _cache:
        case_max, pool = load_pool(shape)
        ks, C, Q, notes = build_batch(shape, pool)
        rows = _file()["%d,%d,%d" % shape]["rows"]
        assert [r[0] for r in rows] == ks.tolist(), "tests/golden/agg_mixed_cases.json is stale: run tests/golden/make_agg_mixed_cases.py"
        acc = np.array([r[1] for r in rows], np.uint8)
        flag = np.array([bool(r[2]) for r in rows])
        for a in (ks, C, Q, acc, flag):
            a.setflags(write=False)
        _cache[key] = (case_max, ks, C, Q, acc, flag, notes)
    return _cache[key]


def uniform_batch(shape, k):
    """The rows of the batch whose ks is k, with the oracle's verdicts: (case_k, ks, C [m, k_max, 64], Q [m, stride], acc, flag)."""
    case_max, ks, C, Q, acc, flag, _ = batch(shape)
    idx = np.flatnonzero(ks == k)
    return setup_on(case_max, k), ks[idx].copy(), np.ascontiguousarray(C[idx]), np.ascontiguousarray(Q[idx]), acc[idx], flag[idx]
