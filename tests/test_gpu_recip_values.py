"""GPU tests of the reciprocal prover from integers (include/bppp.h: bppp_reciprocal_prove_values_batch*): from x, s and the prover's
draws alone -- digits, multiplicities and the value commitment made on the device -- the commitments and proofs equal the
reference-shaped prover's byte for byte at the bit-extraction and the division shapes, across a wavefront boundary; (16, 16) on the
u64 generators equals the u64 prover; the seeded and the device-resident forms equal the host forms, "ct_prover" on or off; an
out-of-range or non-canonical integer flags its own row only; shapes whose digits the integer does not determine are refused."""
import numpy as np
import pytest

import recip_cases

pytestmark = pytest.mark.gpu

SEED = bytes.fromhex("243f6a8885a308d313198a2e03707344a4093822299f31d0082efa98ec4e6c89")
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
SHAPES = [(8, 4, 70), (12, 10, 3), (16, 16, 40), (32, 16, 9)]
_cases, _protos = {}, {}


def _need_gpu():
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")


def _case(nd, npp, B):
    """recip_cases.make(nd, np, B), made once and shared (never written to)."""
    if (nd, npp, B) not in _cases:
        _cases[nd, npp, B] = recip_cases.make(nd, npp, B)
    return _cases[nd, npp, B]


def _proto(nd, npp, B):
    _need_gpu()
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    if (nd, npp) not in _protos:
        case = _case(nd, npp, B)
        _protos[nd, npp] = ReciprocalRangeProofProtocol(nd, npp, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0,
                                                        fb_window_bits=16)
    return _protos[nd, npp]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for p in _protos.values():
        p.close()
    _protos.clear()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _be32(v: int) -> np.ndarray:
    return np.frombuffer(int(v).to_bytes(32, "big"), np.uint8)


@pytest.mark.parametrize("nd,npp,B", SHAPES)
def test_proofs_and_commitments_from_integers_equal_the_reference_shaped_prover(nd, npp, B):
    """From case["x"], case["s"], case["rnd"] alone: commitments == case["commitments"], proofs == case["proofs"] (the oracle's),
    status all zero, every proof accepted.  B = 70 crosses a wavefront; (12, 10) is the division path."""
    case, proto = _case(nd, npp, B), _proto(nd, npp, B)
    proofs, com, st, shape = proto.prove_values_batch(case["label"], case["x"], case["s"], case["rnd"])
    assert shape == (case["rounds"], case["nl"], case["nn"])
    assert not st.any()
    assert (com == case["commitments"]).all()
    assert (proofs == case["proofs"]).all()
    acc, vst = proto.verify_batch(case["label"], com, proofs, *shape)
    assert acc.all() and not vst.any()


def test_u64_dimensions_on_the_u64_generators_equal_the_u64_prover():
    """(16, 16) on a 16 + 32-generator context: bytes equal U64RangeProofProtocol.prove_batch for the same x (both take 52 draws)."""
    _need_gpu()
    import workload
    from bp_pp_amd import U64RangeProofProtocol, draw_scalars
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    n = 70
    x = np.ascontiguousarray(workload.values(n, 4100))
    x[0], x[1], x[2] = 0, (1 << 64) - 1, 0x0123456789ABCDEF
    s = np.ascontiguousarray(workload.blindings(n, 4100))
    rnd = draw_scalars(SEED, 77, n, 52)
    g, gv, hv = workload.split_generators(workload.generators())
    u = U64RangeProofProtocol(g, gv, hv, device=0, fb_window_bits=16)
    try:
        P, V, st = u.prove_batch(x, s, rnd, workload.LABEL)
    finally:
        u.close()
    assert not st.any()
    r = ReciprocalRangeProofProtocol(16, 16, g, gv, hv[:26], [], hv[26:], device=0, fb_window_bits=16)
    try:
        xb = np.stack([_be32(int(v)) for v in x])
        proofs, com, st2, shape = r.prove_values_batch(workload.LABEL, xb, s, rnd)
    finally:
        r.close()
    assert shape == (4, 2, 1) and not st2.any()
    assert (com == V).all() and (proofs == P).all()


@pytest.mark.parametrize("nd,npp,B", [(8, 4, 70), (12, 10, 3)])
def test_seeded_form_equals_the_draws_fed_by_hand_and_the_witness_taking_seeded_prover(nd, npp, B):
    from bp_pp_amd import draw_scalars
    case, proto = _case(nd, npp, B), _proto(nd, npp, B)
    base = (1 << 33) + 5 * nd
    p1, c1, st1, shape = proto.prove_values_batch_seeded(case["label"], case["x"], case["s"], SEED, base)
    p0, c0, st0, _ = proto.prove_values_batch(case["label"], case["x"], case["s"], draw_scalars(SEED, base, B, 20 + 2 * nd))
    assert not st0.any() and not st1.any()
    assert (p1 == p0).all() and (c1 == c0).all() and (c1 == case["commitments"]).all()
    p2, st2, _ = proto.prove_batch_seeded(case["label"], case["commitments"], case["x"], case["s"], case["digits"], case["m"], SEED, base)
    assert not st2.any() and (p1 == p2).all()
    acc, vst = proto.verify_batch(case["label"], c1, p1, *shape)
    assert acc.all() and not vst.any()
    p3, _, _, _ = proto.prove_values_batch_seeded(case["label"], case["x"], case["s"], SEED, base + 1)
    assert all((p3[i] != p1[i]).any() for i in range(B))


@pytest.mark.parametrize("nd,npp,B", [(8, 4, 70), (12, 10, 3)])
def test_device_forms_equal_the_host_forms_with_ct_prover_on_and_off(nd, npp, B):
    """Torch tensors as buffers; nothing is written outside them; "ct_prover" changes no byte."""
    import torch
    case, proto = _case(nd, npp, B), _proto(nd, npp, B)
    pb = proto.proof_bytes()
    base = 900 + nd
    want_p, want_c, want_st, _ = proto.prove_values_batch(case["label"], case["x"], case["s"], case["rnd"])
    seed_p, seed_c, seed_st, _ = proto.prove_values_batch_seeded(case["label"], case["x"], case["s"], SEED, base)
    assert not want_st.any() and not seed_st.any() and (want_p == case["proofs"]).all()
    dX, dS, dR = _dev(case["x"]), _dev(case["s"]), _dev(case["rnd"])
    guard = 64
    for ct in (1, 0, 1, 0):
        proto.set_option("ct_prover", ct)
        try:
            for seeded in (False, True):
                dP = torch.full((B * pb + guard,), 0xA5, dtype=torch.uint8, device="cuda")
                dC = torch.full((B * 64 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
                dSt = torch.full((B + 4,), 77, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                if seeded:
                    proto.prove_values_batch_seeded_device(case["label"], B, dX.data_ptr(), dS.data_ptr(), SEED, base, dP.data_ptr(),
                                                           dC.data_ptr(), dSt.data_ptr())
                else:
                    proto.prove_values_batch_device(case["label"], B, dX.data_ptr(), dS.data_ptr(), dR.data_ptr(), dP.data_ptr(),
                                                    dC.data_ptr(), dSt.data_ptr())
                proto.synchronize()
                gp, gc, gs = dP.cpu().numpy(), dC.cpu().numpy(), dSt.cpu().numpy()
                assert (gp[B * pb:] == 0xA5).all() and (gc[B * 64:] == 0xA5).all() and (gs[B:] == 77).all()
                assert (gp[:B * pb].reshape(B, pb) == (seed_p if seeded else want_p)).all(), (ct, seeded)
                assert (gc[:B * 64].reshape(B, 64) == (seed_c if seeded else want_c)).all(), (ct, seeded)
                assert not gs[:B].any()
            hp, hc, hst, _ = proto.prove_values_batch(case["label"], case["x"], case["s"], case["rnd"])
            assert (hp == want_p).all() and (hc == want_c).all() and not hst.any(), ct
        finally:
            proto.set_option("ct_prover", 0)


def test_flagged_rows_are_zeroed_and_leave_their_wavefront_alone():
    """A batch of 70 at (8, 4): row 5 = 4^8 (out of range), row 64 = n (non-canonical), row 69 = 4^8 - 1 (the largest value in range)."""
    from bp_pp_amd import _capi
    nd, npp, B = 8, 4, 70
    case, proto = _case(nd, npp, B), _proto(nd, npp, B)
    x = case["x"].copy()
    x[5], x[64], x[69] = _be32(4 ** 8), _be32(N), _be32(4 ** 8 - 1)
    proofs, com, st, shape = proto.prove_values_batch(case["label"], x, case["s"], case["rnd"])
    assert int(st[5]) == _capi.ST_OUT_OF_RANGE and int(st[64]) == _capi.ST_BAD_ENCODING
    assert not np.delete(st, [5, 64]).any()
    for row in (5, 64):
        assert not proofs[row].any() and not com[row].any()
    same = [b for b in range(B) if b not in (5, 64, 69)]
    assert (proofs[same] == case["proofs"][same]).all() and (com[same] == case["commitments"][same]).all()
    # row 69: what the witness-taking prover gives for the digits (3, .., 3)
    d69 = np.zeros((1, nd, 32), np.uint8)
    d69[0, :, 31] = 3
    m69 = np.zeros((1, npp, 32), np.uint8)
    m69[0, 3, 31] = nd
    c69, cst = proto.commit_value_batch(x[69:70], case["s"][69:70])
    p69, pst, _ = proto.prove_batch(case["label"], c69, x[69:70], case["s"][69:70], d69, m69, case["rnd"][69:70])
    assert not cst.any() and not pst.any()
    assert (com[69] == c69[0]).all() and (proofs[69] == p69[0]).all()
    ok = [b for b in range(B) if b not in (5, 64)]
    acc, vst = proto.verify_batch(case["label"], com[ok], proofs[ok], *shape)
    assert acc.all() and not vst.any()
    # the device form says the same
    import torch
    dP = torch.full((B, proto.proof_bytes()), 0xA5, dtype=torch.uint8, device="cuda")
    dC = torch.full((B, 64), 0xA5, dtype=torch.uint8, device="cuda")
    dSt = torch.full((B,), 77, dtype=torch.int32, device="cuda")
    dX, dS, dR = _dev(x), _dev(case["s"]), _dev(case["rnd"])
    torch.cuda.synchronize()
    proto.prove_values_batch_device(case["label"], B, dX.data_ptr(), dS.data_ptr(), dR.data_ptr(), dP.data_ptr(), dC.data_ptr(), dSt.data_ptr())
    proto.synchronize()
    assert (dP.cpu().numpy() == proofs).all() and (dC.cpu().numpy() == com).all() and (dSt.cpu().numpy() == st).all()


def test_shapes_the_integer_does_not_determine_are_refused_before_any_launch():
    """(256, 16) and (64, 16) on a context large enough for both: BPPP_ERR_INVALID_ARG, nothing launched, every output as it was.
    The witness-taking prover keeps serving such a shape."""
    _need_gpu()
    from bp_pp_amd import BpppError, _capi
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    case = recip_cases.make(256, 16, 1, n_oracle=0)
    big = ReciprocalRangeProofProtocol(256, 16, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0, fb_window_bits=8)
    try:
        big.enable_timing(True)
        big.timings(reset=True)
        for nd in (256, 64):
            proto = big if nd == 256 else ReciprocalRangeProofProtocol.borrowed(64, 16, big._w._ctx.value, big._w.ng, big._w.nh)
            assert not proto.values_shape_ok()
            B = 2
            x, s = np.zeros((B, 32), np.uint8), np.ones((B, 32), np.uint8)
            rnd = np.ones((B, 20 + 2 * nd, 32), np.uint8)
            proofs, com = np.full((B, proto.proof_bytes()), 0xA5, np.uint8), np.full((B, 64), 0xA5, np.uint8)
            st = np.full(B, 77, np.int32)
            L = _capi.lib()
            rc = L.bppp_reciprocal_prove_values_batch(proto._w._ctx, case["label"], len(case["label"]), B, nd, 16, x.ctypes.data,
                                                      s.ctypes.data, rnd.ctypes.data, proofs.ctypes.data, com.ctypes.data, st.ctypes.data)
            assert rc == _capi.ERR_INVALID_ARG
            rc = L.bppp_reciprocal_prove_values_batch_seeded(proto._w._ctx, case["label"], len(case["label"]), B, nd, 16, x.ctypes.data,
                                                             s.ctypes.data, SEED, 0, proofs.ctypes.data, com.ctypes.data, st.ctypes.data)
            assert rc == _capi.ERR_INVALID_ARG
            assert (st == 77).all() and (proofs == 0xA5).all() and (com == 0xA5).all()
            with pytest.raises(BpppError) as e:
                proto.prove_values_batch(case["label"], x, s, rnd)
            assert e.value.code == _capi.ERR_INVALID_ARG
        assert not any(v["launches"] for v in big.timings(reset=True).values())
        # the shape itself is served from a witness, as before
        com, cst = big.commit_value_batch(case["x"], case["s"])
        p, pst, shape = big.prove_batch(case["label"], com, case["x"], case["s"], case["digits"], case["m"], case["rnd"])
        big.enable_timing(False)
        acc, vst = big.verify_batch(case["label"], com, p, *shape)
        assert not cst.any() and not pst.any() and acc.all() and not vst.any()
    finally:
        big.close()
