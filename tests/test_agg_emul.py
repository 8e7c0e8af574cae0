"""CPU tier for the aggregated reciprocal range proof verifier's device code (bp_pp_amd/csrc/agg_core.h compiled for the host,
tests/emul/agg_emul.cpp): agg_phase1 -- one lane and as G runs summed on the host --, both halves of C0 and the finish, then the
WNLA stage, against the oracle: rho, mu, the whole c vector, ps_tau, pn_tau, C0 and the status bit for bit with the oracle's trace,
and the verdicts of the corrupted batch (tests/agg_cases.py: corrupted_batch) with the golden file's."""
import numpy as np
import pytest

import agg_cases as A
import agg_golden
import bppp_oracle as O
from emul.build import load as load_emul
from emul.build_agg import load as load_agg

W = 4
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


def run(case, C, Q, G=1, slow=0):
    L = load_agg()
    n, k, nm, NH = C.shape[0], case["k"], case["nm"], case["NH"]
    C, Q = np.ascontiguousarray(C), np.ascontiguousarray(Q)
    assert Q.shape == (n, case["proof_bytes"])
    out = dict(rho=np.zeros((n, 32), np.uint8), mu=np.zeros((n, 32), np.uint8), c=np.zeros((n, NH, 32), np.uint8),
               pn=np.zeros((n, nm + 1, 32), np.uint8), c0=np.zeros((n, 64), np.uint8), p1=np.zeros(n, np.int32),
               acc=np.zeros(n, np.uint8), st=np.zeros(n, np.int32))
    tab = _table(case)
    rc = L.emul_agg_verify(tab.ctypes.data, W, case["NG"], NH, k, case["nd"], case["np"], case["label"], len(case["label"]), n,
                           C.ctypes.data, Q.ctypes.data, case["rounds"], case["nl"], case["nn"], G, slow, out["rho"].ctypes.data,
                           out["mu"].ctypes.data, out["c"].ctypes.data, out["pn"].ctypes.data, out["c0"].ctypes.data, out["p1"].ctypes.data,
                           out["acc"].ctypes.data, out["st"].ctypes.data)
    assert rc == 0
    return out


def _sc(row):
    return int.from_bytes(row.tobytes(), "big")


def _assert_trace(case, out, i, com, proof):
    tr = []
    assert A.verify(case, com, proof, tr) == 1
    d = {k: v for k, v in tr if not k.startswith("wnla")}
    assert _sc(out["rho"][i]) == d["rho"] and _sc(out["mu"][i]) == d["rho"] * d["rho"] % O.N
    assert [_sc(r) for r in out["c"][i]] == d["c"]
    assert _sc(out["pn"][i, 0]) == d["ps_tau"] and [_sc(r) for r in out["pn"][i, 1:]] == d["pn_tau"]
    assert out["c0"][i].tobytes() == O.pt_to_xy64(d["C0"])
    assert out["p1"][i] == 0 and out["acc"][i] == 1 and out["st"][i] == 0


@pytest.mark.parametrize("shape", [s for s in A.SHAPES if s != (16, 16, 16)])
def test_phase1_c0_and_verdict_equal_the_oracle_trace(shape):
    case, coms, proofs, _ = agg_golden.load(shape)
    out = run(case, coms, proofs)
    for i in range(len(proofs)):
        _assert_trace(case, out, i, coms[i].tobytes(), proofs[i].tobytes())


def test_the_16_value_u64_shape_equals_the_oracle_trace():
    """(16, 16, 16): |g_vec| = 256, |h_vec| = 26 padded to 32, 6 rounds, 2,208 bytes for 16 values."""
    case, coms, proofs, _ = agg_golden.load((16, 16, 16))
    assert (case["NG"], case["NH"], case["rounds"], case["nl"], case["nn"], case["proof_bytes"]) == (256, 32, 6, 1, 4, 2208)
    out = run(case, coms, proofs)
    assert out["acc"].tolist() == [1, 1, 1] and not out["st"].any()
    _assert_trace(case, out, 2, coms[2].tobytes(), proofs[2].tobytes())
    for G in (2, 8):
        o = run(case, coms, proofs, G=G)
        assert all((o[key] == out[key]).all() for key in out), G


@pytest.mark.parametrize("shape", [(2, 4, 4), (3, 4, 4), (6, 2, 3), (7, 3, 4)])
def test_lane_group_runs_sum_to_the_one_lane_result(shape):
    """G = 2, 4, 8 runs of consecutive entries, each starting its powers at its own exponents (runs cross value boundaries: nd = 2, 3,
    4 against run lengths 1 .. 11; G = 8 > k nd leaves empty runs at (2, 4, 4) only by one), summed on the host: every output byte
    equals the one-lane form's, on clean and on corrupted rows."""
    case, C, Q, _, _, _ = agg_golden.batch(shape)
    C, Q = C[:24], Q[:24]
    ref = run(case, C, Q)
    for G in (2, 4, 8):
        o = run(case, C, Q, G=G)
        for key in ref:
            assert (o[key] == ref[key]).all(), (shape, G, key)


@pytest.mark.parametrize("shape", [s for s in A.SHAPES if s != (16, 16, 16)])
def test_corrupted_rows_get_the_oracle_verdicts_on_both_c0_paths(shape):
    """Every field class corrupted, V_i = R_i and V_i = -R_i included: accept and status as the oracle's (golden file), on the affine
    window tables and on the projective-table form."""
    case, C, Q, acc, flag, kinds = agg_golden.batch(shape)
    for slow in (0, 1):
        o = run(case, C, Q, slow=slow)
        assert (o["acc"] == acc).all(), (shape, slow, [(r, kind) for r, kind in kinds if o["acc"][r] != acc[r]])
        assert ((o["st"] != 0) == flag).all() and ((o["st"] & 1 != 0) == flag).all(), (shape, slow, o["st"].tolist())
        assert ((o["p1"] != 0) == flag).all()      # every malformed row here is malformed in a point phase 1 decodes


def test_sums_that_meet_the_exceptions_of_the_group_law():
    """V_i = R_i (a doubling), V_i = -R_i (the identity: hashed as 33 zero bytes) and V_i = identity, in the first, a middle and the
    last value: C0 and the verdict are the oracle's."""
    shape = (3, 4, 4)
    case, coms, proofs, _ = agg_golden.load(shape)
    k, off = case["k"], A.field_offsets(case)["R_first"]
    C, Q = np.repeat(coms[:1], 9, axis=0), np.repeat(proofs[:1], 9, axis=0)
    for i in range(k):
        C[i, i] = Q[i, off + 64 * i:off + 64 * i + 64]
        C[3 + i, i] = np.frombuffer(A.neg_point(Q[3 + i, off + 64 * i:off + 64 * i + 64].tobytes()), np.uint8)
        C[6 + i, i] = 0
    o = run(case, C, Q)
    for r in range(9):
        tr = []
        rc = A.verify(case, C[r].tobytes(), Q[r].tobytes(), tr)
        d = dict(tr)
        assert rc == 0 and o["acc"][r] == 0 and o["st"][r] == 0
        assert o["c0"][r].tobytes() == O.pt_to_xy64(d["C0"]), r
        assert [_sc(x) for x in o["c"][r]] == d["c"]
    assert dict(tr)["V+R"][2] == O.pt_from_xy64(Q[8, off + 128:off + 192].tobytes())
