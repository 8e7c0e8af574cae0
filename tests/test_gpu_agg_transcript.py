"""The aggregated reciprocal range proof on the CALLER'S transcripts on the GPU (bppp_reciprocal_agg_verify_batch_transcript[_device|_sec1],
bppp_reciprocal_agg_prove_values_batch_transcript[_seeded|_device]) against the oracle on the same pre-loaded transcripts
(tests/golden/agg_transcript_cases.json, made by tests/golden/make_agg_transcript_cases.py from tests/agg_transcript_cases.py).
Every comparison is bit-exact: accept, status, reject count, and the 203 bytes of every advanced state.

Shapes (k, nd, np): (2, 4, 4) the smallest aggregate; (3, 4, 4) nm padded; (6, 2, 3) np = nd + 1, ten C0 points; (16, 16, 16) sixteen
u64 values -- 16 appends before the first challenge, the sponge wraps several times -- once, over a dozen rows.
State layouts: one shared state; n states at one position; n states at MIXED positions -- six positions cycling row by row, so that
every wavefront holds all six and neighbouring lanes differ: the lowest a pre-loaded state can have (0), 165, 150 and 163 (the first
reciprocal_commitment append crosses the rate boundary inside its meta-AD), 120 and 136 (inside its 33 data bytes).
Rows 6 .. 9 of a mixed batch are corrupted, one per field class (a wrong-but-valid point, a scalar bit, swapped V, an off-curve R)."""
import json
import os

import numpy as np
import pytest

import agg_cases as A
import agg_prove_cases as AP
import agg_transcript_cases as AT
from bp_pp_amd import wire

pytestmark = pytest.mark.gpu

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_transcript_cases.json")
SEED = bytes.fromhex("243f6a8885a308d313198a2e03707344a4093822299f31d0082efa98ec4e6c89")
ROWS = {(16, 16, 16): 12}            # rows of a batch (default 70: a full wavefront and a ragged one)
_golden, _made = {}, {}


def _u8(blobs, *shape):
    return np.frombuffer(b"".join(blobs), np.uint8).reshape(len(blobs), *shape).copy()


def golden(shape):
    """-> dict(case, mixed / shared: (b, C [P, k, 64], Q [P, pb], S_in [P, 203], S_out [P, 203]), corrupted, rebound); never written to."""
    if shape not in _golden:
        if "file" not in _golden:
            with open(PATH) as f:
                _golden["file"] = json.load(f)
        g = _golden["file"]["%d,%d,%d" % shape]
        case = A.setup(*shape)
        assert (g["rounds"], g["nl"], g["nn"]) == (case["rounds"], case["nl"], case["nn"])
        out = dict(case=case, corrupted=g["corrupted"], rebound=g["rebound"])
        for pool, state_of in (("mixed", lambda i: AT.mixed_state(case, i)), ("shared", lambda i: AT.shared_state(case))):
            es = g[pool]
            out[pool] = ([e["b"] for e in es], _u8([bytes.fromhex(e["commitments"]) for e in es], shape[0], 64),
                         _u8([bytes.fromhex(e["proof"]) for e in es], case["proof_bytes"]), _u8([state_of(i) for i in range(len(es))], 203),
                         _u8([bytes.fromhex(e["state_out"]) for e in es], 203))
        _golden[shape] = out
    return _golden[shape]


def batch(shape, pool, n=None, corrupt=True):
    """n rows cycling through the pool -> (case, C, Q, S_in [n, 203], accept, flagged, S_out [n, 203]); rows 6 .. 9 of the mixed pool
    corrupted by class, with the oracle's verdict and state."""
    g = golden(shape)
    n = n or ROWS.get(shape, 70)
    _, C, Q, Si, So = g[pool]
    idx = np.arange(n) % len(C)
    C, Q, Si, So = (np.ascontiguousarray(a[idx]) for a in (C, Q, Si, So))
    acc, flag = np.ones(n, np.uint8), np.zeros(n, bool)
    if pool == "mixed" and corrupt:
        for entry, kind, a, f, sout in g["corrupted"]:
            row = len(g["mixed"][1]) + entry
            assert idx[row] == entry
            AT.corrupt(g["case"], C[row], Q[row], kind)
            acc[row], flag[row], So[row] = a, bool(f), np.frombuffer(bytes.fromhex(sout), np.uint8)
            if f:
                assert So[row].tobytes() == Si[row].tobytes()      # the oracle leaves a transcript it could not start on untouched
    return g["case"], C, Q, Si, acc, flag, So


def _proto(shape, **env):
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol
    key = (shape, tuple(sorted(env.items())))
    if key not in _made:
        case = golden(shape)["case"] if shape[0] > 1 else A.setup(*shape)
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            _made[key] = AggregatedReciprocalRangeProofProtocol(shape[0], shape[1], shape[2], case["g"], case["gv"], case["hv"], case["gv_"],
                                                                case["hv_"], device=0, fb_window_bits=8)
    return _made[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for p in _made.values():
        p.close()
    _made.clear()


def _device_verify(v, case, C, Q, S):
    import torch
    n = C.shape[0]
    dC, dQ, dS = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (C, Q, S))
    dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dSt = torch.full((n,), 7, dtype=torch.int32, device="cuda")          # (an instance no kernel reached keeps the 7)
    dR = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    dO = torch.full((n, 203), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    v.verify_batch_transcript_device(n, dS.data_ptr(), S.shape[0], dC.data_ptr(), dQ.data_ptr(), case["rounds"], case["nl"], case["nn"],
                                     dA.data_ptr(), dSt.data_ptr(), dR.data_ptr(), dO.data_ptr())
    v.synchronize()
    torch.cuda.synchronize()
    return dA.cpu().numpy(), dSt.cpu().numpy(), int(dR.cpu()[0]), dO.cpu().numpy()


def _assert_rows(got, acc, flag, So, tag):
    g_acc, g_st, g_out = got
    wrong = np.flatnonzero(g_acc != acc)
    assert wrong.size == 0, (tag, "accept bits differ at", wrong[:16].tolist())
    wrong = np.flatnonzero(g_st != np.where(flag, AT.ST_BAD_ENCODING, 0))
    assert wrong.size == 0, (tag, "statuses differ at", wrong[:16].tolist(), g_st[wrong[:16]].tolist())
    wrong = np.flatnonzero((g_out != So).any(axis=1))
    assert wrong.size == 0, (tag, "states_out differ at", wrong[:16].tolist())


def _all_forms(v, case, C, Q, S, acc, flag, So, tag):
    rounds, nl, nn, k = case["rounds"], case["nl"], case["nn"], case["k"]
    _assert_rows(v.verify_batch_transcript(S, C, Q, rounds, nl, nn), acc, flag, So, (tag, "host"))
    d = _device_verify(v, case, C, Q, S)
    _assert_rows((d[0], d[1], d[3]), acc, flag, So, (tag, "device"))
    assert d[2] == int((acc == 0).sum()), (tag, "reject count")
    n = C.shape[0]
    C33 = wire.pack(C.reshape(n, -1), k).reshape(n, k, 33)
    Q33 = wire.pack(Q, 4 + 2 * rounds + k, nl + nn)
    # compression keeps x and the parity of y, so the off-curve R of the 64-byte batch would come back ON the curve: in the wire form
    # that row's R carries a tag no SEC1 point has, which is the wire form's off-curve point (BPPP_ST_BAD_ENCODING, state returned)
    for row in np.flatnonzero(flag):
        Q33[row, 33 * (4 + 2 * rounds + k // 2)] = 5
    _assert_rows(v.verify_batch_transcript_sec1(S, C33, Q33, rounds, nl, nn), acc, flag, So, (tag, "sec1"))


@pytest.mark.parametrize("shape", AT.SHAPES)
def test_mixed_positions_every_corrupted_class_host_device_sec1(shape):
    case, C, Q, S, acc, flag, So = batch(shape, "mixed")
    pos = S[:, 200]
    assert len(set(pos[:64].tolist())) >= 5 and (pos[1:] != pos[:-1]).all()
    assert {0, 165} <= set(pos.tolist()) and AT.lowest_position(case["label"]) == 0
    assert flag.sum() == 1 and (acc == 0).sum() == 4
    _all_forms(_proto(shape), case, C, Q, S, acc, flag, So, (shape, "mixed"))


@pytest.mark.parametrize("shape", AT.SHAPES)
def test_one_shared_state_and_n_equal_states(shape):
    case, C, Q, S, acc, flag, So = batch(shape, "shared")
    assert (S == S[0]).all()
    v = _proto(shape)
    _all_forms(v, case, C, Q, S[:1], acc, flag, So, (shape, "n_states = 1"))
    _all_forms(v, case, C, Q, S, acc, flag, So, (shape, "n_states = n"))


def test_an_invalid_state_does_not_disturb_its_wavefront():
    """Rows whose byte 200 is >= 166 among valid rows: the first lane of a wavefront, one whose byte 200 is the label state's position
    (42) with byte 201 out of range, one in the ragged last wavefront.  The device form flags exactly those and returns them
    unchanged; the host form refuses the call."""
    from bp_pp_amd import _capi
    shape = (2, 4, 4)
    case, C, Q, S, acc, flag, So = batch(shape, "mixed", 134)
    label_pos = AT.ser(AT.O.Transcript(case["label"]))[200]
    bad = {64: (200, 166), 3: (200, 255), 65: (201, 167), 133: (200, 200)}
    for row, (byte, val) in bad.items():
        if row == 65:
            S[row, 200] = label_pos
        S[row, byte] = val
        acc[row], flag[row], So[row] = 0, True, S[row]
    v = _proto(shape)
    d = _device_verify(v, case, C, Q, S)
    _assert_rows((d[0], d[1], d[3]), acc, flag, So, "invalid states, device")
    assert d[2] == int((acc == 0).sum())
    with pytest.raises(_capi.BpppError) as e:
        v.verify_batch_transcript(S, C, Q, case["rounds"], case["nl"], case["nn"])
    assert e.value.code == _capi.ERR_INVALID_ARG


def test_launch_forms_are_the_label_paths():
    """Phase 1 on one lane (n = 32 S + 1), on eight (a small n), and on two by BPPP_GENERIC_LANE_GROUP=2 on (16, 16, 16), whose runs
    cross value boundaries: the form recorded is the one the label path records at that size."""
    shape = (2, 4, 4)
    v = _proto(shape)
    S_ = v.get_option("n_simds")
    for n, group in ((32 * S_ + 1, 1), (70, 8)):
        case, C, Q, S, acc, flag, So = batch(shape, "mixed", n)
        d = _device_verify(v, case, C, Q, S)
        form = v._w.generic_form()
        _assert_rows((d[0], d[1], d[3]), acc, flag, So, ("launch form", n))
        assert form["phase1_group"] == group and form["protocol"] == "aggregate", form
        v.verify_batch(case["label"], C, Q, case["rounds"], case["nl"], case["nn"])
        assert v._w.generic_form() == form, (n, "the label path's form")
    shape = (16, 16, 16)
    v = _proto(shape, BPPP_GENERIC_LANE_GROUP="2")
    case, C, Q, S, acc, flag, So = batch(shape, "mixed")
    d = _device_verify(v, case, C, Q, S)
    _assert_rows((d[0], d[1], d[3]), acc, flag, So, "lane group 2")
    form = v._w.generic_form()
    assert form["phase1_group"] == 2 and form["protocol"] == "aggregate", form
    v.verify_batch(case["label"], C, Q, case["rounds"], case["nl"], case["nn"])
    assert v._w.generic_form() == form, "the label path's form"


@pytest.mark.parametrize("shape", AT.SHAPES[:3])
def test_a_proof_bound_to_one_transcript_is_rejected_under_another(shape):
    g = golden(shape)
    case = g["case"]
    _, C, Q, Si, _ = g["mixed"]
    r_acc, r_flag, r_out = g["rebound"]
    assert r_acc == 0 and r_flag == 0                       # the oracle rejects too
    got = _proto(shape).verify_batch_transcript(Si[1:2], C[0:1], Q[0:1], case["rounds"], case["nl"], case["nn"])
    _assert_rows(got, np.zeros(1, np.uint8), np.zeros(1, bool), _u8([bytes.fromhex(r_out)], 203), "rebound")


def test_k1_is_the_reciprocal_transcript_verifier():
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    shape = (1, 4, 4)
    import agg_golden
    case, Cg, Qg, exp_acc, exp_flag, _ = agg_golden.batch(shape)
    S = _u8([AT.mixed_state(case, i) for i in range(A.ROWS)], 203)
    r = ReciprocalRangeProofProtocol(4, 4, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0, fb_window_bits=8)
    try:
        want = r.verify_batch(b"", Cg.reshape(A.ROWS, 64), Qg, case["rounds"], case["nl"], case["nn"], transcripts=S)
    finally:
        r.close()
    v = _proto(shape)
    got = v.verify_batch_transcript(S, Cg, Qg, case["rounds"], case["nl"], case["nn"])
    d = _device_verify(v, case, Cg, Qg, S)
    for a, b in zip(want, got):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    assert d[0].tobytes() == got[0].tobytes() and d[1].tobytes() == got[1].tobytes() and d[3].tobytes() == got[2].tobytes()
    assert d[2] == int((got[0] == 0).sum()) and (got[1] != 0).sum() == exp_flag.sum()


def test_parts_of_max_batch_carry_their_own_states():
    shape = (3, 4, 4)
    v = _proto(shape)
    case, C, Q, S, acc, flag, So = batch(shape, "mixed", 1024 + 70)
    before = v.get_option("max_batch")
    v.set_option("max_batch", 1024)
    try:
        _assert_rows(v.verify_batch_transcript(S, C, Q, case["rounds"], case["nl"], case["nn"]), acc, flag, So, "host parts")
        d = _device_verify(v, case, C, Q, S)
        _assert_rows((d[0], d[1], d[3]), acc, flag, So, "device parts")
        assert d[2] == int((acc == 0).sum())
    finally:
        v.set_option("max_batch", before)


def test_argument_refusals():
    from bp_pp_amd import _capi
    shape = (2, 4, 4)
    v = _proto(shape)
    case, C, Q, S, *_ = batch(shape, "mixed", 16)
    L, E, p = _capi.lib(), _capi.ERR_INVALID_ARG, C.ctypes.data
    f = L.bppp_reciprocal_agg_verify_batch_transcript
    tail = (p, p, case["rounds"], case["nl"], case["nn"], p, p, p)
    assert f(v._w._ctx, 8, p, 3, 2, 4, 4, *tail) == E            # n_states neither 1 nor n
    assert f(v._w._ctx, 8, None, 8, 2, 4, 4, *tail) == E         # NULL states
    assert f(v._w._ctx, 0, p, 1, 0, 4, 4, *tail) == E            # k out of range, n = 0
    assert f(v._w._ctx, 0, p, 1, 65, 4, 4, *tail) == E
    g = L.bppp_reciprocal_agg_prove_values_batch_transcript
    assert g(v._w._ctx, 8, p, 3, 2, 4, 4, p, p, p, p, p, p, p) == E
    assert g(v._w._ctx, 0, p, 1, 0, 4, 4, p, p, p, p, p, p, p) == E


# ---------------------------------------------------------------- the prover
def _prove_inputs(shape, pool, n=None):
    g = golden(shape)
    bs, C, Q, Si, So = g[pool]
    n = n or len(bs)
    idx = np.arange(n) % len(bs)
    x, s, rnd = AP.batch(g["case"], [bs[i] for i in idx], _proto(shape).prove_draws())
    return g["case"], x, s, rnd, np.ascontiguousarray(Si[idx]), np.ascontiguousarray(C[idx]), np.ascontiguousarray(Q[idx]), np.ascontiguousarray(So[idx])


def _device_prove(p, S, x, s, rnd):
    import torch
    n = x.shape[0]
    dx, ds, dr, dS = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, s, rnd, S))
    pb = p.proof_bytes(*p.proof_shape())
    dP = torch.full((n, pb), 0xEE, dtype=torch.uint8, device="cuda")
    dC = torch.full((n, p.k, 64), 0xEE, dtype=torch.uint8, device="cuda")
    dSt = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    dO = torch.full((n, 203), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p.prove_values_batch_transcript_device(n, dS.data_ptr(), S.shape[0], dx.data_ptr(), ds.data_ptr(), dr.data_ptr(), dP.data_ptr(), dC.data_ptr(),
                                           dSt.data_ptr(), dO.data_ptr())
    p.synchronize()
    torch.cuda.synchronize()
    return dP.cpu().numpy(), dC.cpu().numpy(), dSt.cpu().numpy(), dO.cpu().numpy()


@pytest.mark.parametrize("shape", AT.SHAPES)
def test_prover_bytes_and_states_equal_the_oracles_shared_and_mixed(shape):
    p = _proto(shape)
    n = {(16, 16, 16): None}.get(shape, 70)
    for pool in ("mixed", "shared"):
        case, x, s, rnd, Si, C, Q, So = _prove_inputs(shape, pool, n)
        states = Si[:1] if pool == "shared" else Si
        got, gcom, st, _, out = p.prove_values_batch_transcript(states, x, s, rnd)
        assert not st.any(), st.tolist()
        assert gcom.tobytes() == C.tobytes() and got.tobytes() == Q.tobytes(), (shape, pool, "proofs")
        assert out.tobytes() == So.tobytes(), (shape, pool, "states_out")
        dP, dC, dSt, dO = _device_prove(p, states, x, s, rnd)
        assert dP.tobytes() == got.tobytes() and dC.tobytes() == gcom.tobytes() and not dSt.any() and dO.tobytes() == out.tobytes()


def test_seeded_prover_equals_the_host_form_on_its_draws():
    from bp_pp_amd.range_proof import draw_scalars
    shape = (2, 4, 4)
    p = _proto(shape)
    case, x, s, _, Si, *_ = _prove_inputs(shape, "mixed", 70)
    rnd = draw_scalars(SEED, 1000, 70, p.prove_draws())
    want = p.prove_values_batch_transcript(Si, x, s, rnd)
    got = p.prove_values_batch_transcript_seeded(Si, x, s, SEED, 1000)
    assert not want[2].any()
    for a, b in zip((want[0], want[1], want[2], want[4]), (got[0], got[1], got[2], got[4])):
        assert a.tobytes() == b.tobytes()


def test_flagged_instance_is_zeroed_gets_its_state_back_and_round_trip():
    """One out-of-range value in the batch: zeroed, flagged, its input state back, the neighbours untouched.  Then the GPU's proofs on
    pre-loaded transcripts through the GPU verifier on the same states (and, for the golden rows, they ARE the oracle's bytes, which
    the oracle accepts: tests/golden/make_agg_transcript_cases.py): both states_out agree."""
    shape = (2, 4, 4)
    p = _proto(shape)
    case, x, s, rnd, Si, C, Q, So = _prove_inputs(shape, "mixed", 70)
    row = 65
    x = x.copy()
    x[row, 1] = np.frombuffer((4**4).to_bytes(32, "big"), np.uint8)
    got, gcom, st, (rounds, nl, nn), out = p.prove_values_batch_transcript(Si, x, s, rnd)
    keep = np.arange(70) != row
    assert st[row] == AT.ST_OUT_OF_RANGE and not st[keep].any()
    assert not got[row].any() and not gcom[row].any() and out[row].tobytes() == Si[row].tobytes()
    assert got[keep].tobytes() == Q[keep].tobytes() and gcom[keep].tobytes() == C[keep].tobytes() and out[keep].tobytes() == So[keep].tobytes()
    acc, vst, vout = p.verify_batch_transcript(Si, gcom, got, rounds, nl, nn)
    assert acc[keep].all() and not vst[keep].any() and vout[keep].tobytes() == out[keep].tobytes()
    assert acc[row] == 0


def test_device_prover_flags_invalid_states_among_valid_ones():
    """Rows whose state merlin cannot be in -- the first lane of a wavefront, one at the label state's position with byte 201 out of
    range, one in the ragged last wavefront -- among valid rows at mixed positions: the device form flags exactly those
    BPPP_ST_BAD_ENCODING, zeroes their proofs and commitments and returns their states unchanged; every other row is the oracle's.
    The host forms refuse the call."""
    from bp_pp_amd import _capi
    shape = (2, 4, 4)
    p = _proto(shape)
    case, x, s, rnd, Si, C, Q, So = _prove_inputs(shape, "mixed", 134)
    Si = Si.copy()
    label_pos = AT.ser(AT.O.Transcript(case["label"]))[200]
    bad = {64: (200, 166), 3: (200, 255), 65: (201, 167), 133: (200, 200)}
    for row, (byte, val) in bad.items():
        if row == 65:
            Si[row, 200] = label_pos
        Si[row, byte] = val
    dP, dC, dSt, dO = _device_prove(p, Si, x, s, rnd)
    rows = sorted(bad)
    keep = np.setdiff1d(np.arange(134), rows)
    assert (dSt[rows] == AT.ST_BAD_ENCODING).all() and not dSt[keep].any(), dSt.tolist()
    assert not dP[rows].any() and not dC[rows].any() and dO[rows].tobytes() == Si[rows].tobytes()
    assert dP[keep].tobytes() == Q[keep].tobytes() and dC[keep].tobytes() == C[keep].tobytes() and dO[keep].tobytes() == So[keep].tobytes()
    for call in (lambda: p.prove_values_batch_transcript(Si, x, s, rnd), lambda: p.prove_values_batch_transcript_seeded(Si, x, s, SEED, 5)):
        with pytest.raises(_capi.BpppError) as e:
            call()
        assert e.value.code == _capi.ERR_INVALID_ARG


def test_k1_prover_is_the_reciprocal_prover_from_integers_on_the_callers_transcript():
    """k = 1 of the three prover forms goes through the reciprocal prover from integers: on the label's own state its bytes are
    bppp_reciprocal_prove_values_batch's; on pre-loaded states proofs, commitments and states are the oracle's; host, seeded and
    device forms agree; a flagged row (out of range; in the device form an invalid state) is zeroed and gets its state back."""
    from bp_pp_amd.range_proof import draw_scalars
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    shape = (1, 4, 4)
    case = A.setup(*shape)
    p = _proto(shape)
    n = 70
    bs = [i % 5 for i in range(n)]
    x, s, rnd = AP.batch(case, bs, p.prove_draws())
    S = _u8([AT.mixed_state(case, i) for i in range(n)], 203)
    got, gcom, st, (rounds, nl, nn), out = p.prove_values_batch_transcript(S, x, s, rnd)
    assert not st.any(), st.tolist()
    for i in (0, 1, 2, 9, 69):                                   # the oracle on the same transcript and draws
        c, q, so = AT.prove_state(case, S[i].tobytes(), bs[i])
        assert gcom[i].tobytes() == c and got[i].tobytes() == q and out[i].tobytes() == so, i
    acc, vst, vout = p.verify_batch_transcript(S, gcom, got, rounds, nl, nn)
    assert acc.all() and not vst.any() and vout.tobytes() == out.tobytes()
    # the label's own state: the reciprocal prover from integers, byte for byte
    S0 = _u8([AT.ser(AT.O.Transcript(case["label"]))], 203)
    r = ReciprocalRangeProofProtocol(4, 4, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0, fb_window_bits=8)
    try:
        rp, rc, rst, _ = r.prove_values_batch(case["label"], x.reshape(-1, 32), s.reshape(-1, 32), rnd)
    finally:
        r.close()
    lp, lc, lst, _, _ = p.prove_values_batch_transcript(S0, x, s, rnd)
    assert lp.tobytes() == rp.tobytes() and lc.tobytes() == rc.tobytes() and lst.tobytes() == rst.tobytes()
    # seeded = the host form on the seed's draws
    drawn = draw_scalars(SEED, 40, n, p.prove_draws())
    want = p.prove_values_batch_transcript(S, x, s, drawn)
    seeded = p.prove_values_batch_transcript_seeded(S, x, s, SEED, 40)
    for a, b in zip((want[0], want[1], want[2], want[4]), (seeded[0], seeded[1], seeded[2], seeded[4])):
        assert a.tobytes() == b.tobytes()
    # device = host; with one out-of-range value and one invalid state
    x2, S2 = x.copy(), S.copy()
    x2[7, 0] = np.frombuffer((4**4).to_bytes(32, "big"), np.uint8)
    hp, hc, hst, _, hout = p.prove_values_batch_transcript(S2, x2, s, rnd)
    assert hst[7] == AT.ST_OUT_OF_RANGE and not hp[7].any() and not hc[7].any() and hout[7].tobytes() == S2[7].tobytes()
    keep = np.arange(n) != 7
    assert hp[keep].tobytes() == got[keep].tobytes() and hout[keep].tobytes() == out[keep].tobytes() and not hst[keep].any()
    S2[64, 200] = 170
    dP, dC, dSt, dO = _device_prove(p, S2, x2, s, rnd)
    keep = np.setdiff1d(np.arange(n), [7, 64])
    assert dSt[7] == AT.ST_OUT_OF_RANGE and dSt[64] == AT.ST_BAD_ENCODING and not dSt[keep].any()
    assert not dP[[7, 64]].any() and not dC[[7, 64]].any() and dO[[7, 64]].tobytes() == S2[[7, 64]].tobytes()
    assert dP[keep].tobytes() == got[keep].tobytes() and dC[keep].tobytes() == gcom[keep].tobytes() and dO[keep].tobytes() == out[keep].tobytes()
