"""The aggregated reciprocal range proof PROVER on the GPU (bppp_reciprocal_agg_prove_values_batch*; csrc/agg_prove_core.h,
k_aggprove.hip): k integers per instance in, k value commitments and one proof out.  Every comparison is bit-exact.

The expected bytes are the oracle's golden proofs (tests/golden/agg_cases.json); tests/agg_prove_cases.py rebuilds the x, s and draws the
oracle's prover was fed, so no test here runs the Python prover.  Shapes (k, nd, np) as tests/test_gpu_agg.py: (1, 4, 4) is the
reciprocal prover from integers, (6, 2, 3) has np = nd + 1, (7, 3, 4) pads nm = 21 to 32, (16, 16, 16) is sixteen u64 values.  Batches of
70 rows cross a wavefront boundary with a ragged last block."""
import numpy as np
import pytest

import agg_cases as A
import agg_golden
import agg_prove_cases as AP

pytestmark = pytest.mark.gpu

SEED = bytes.fromhex("243f6a8885a308d313198a2e03707344a4093822299f31d0082efa98ec4e6c89")
ST_BAD_ENCODING, ST_OUT_OF_RANGE = 1, 4
ROWS = 70
_made, _inputs = {}, {}


def _proto(shape):
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol
    if shape not in _made:
        case = agg_golden.load(shape)[0]
        _made[shape] = AggregatedReciprocalRangeProofProtocol(shape[0], shape[1], shape[2], case["g"], case["gv"], case["hv"], case["gv_"],
                                                              case["hv_"], device=0, fb_window_bits=8)
    return _made[shape]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for p in _made.values():
        p.close()
    _made.clear()


def _golden_inputs(shape):
    """(case, commitments, proofs, x, s, rnd) of the shape's golden instances, made once and never written to."""
    if shape not in _inputs:
        case, coms, proofs, _ = agg_golden.load(shape)
        x, s, rnd = AP.batch(case, range(len(proofs)), _proto(shape).prove_draws())
        _inputs[shape] = (case, coms, proofs, x, s, rnd)
    return _inputs[shape]


def _rows(shape, n):
    """n rows of valid inputs: the golden instances repeated."""
    case, coms, proofs, x, s, rnd = _golden_inputs(shape)
    idx = np.arange(n) % len(proofs)
    return case, np.ascontiguousarray(x[idx]), np.ascontiguousarray(s[idx]), np.ascontiguousarray(rnd[idx]), idx


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out(p, n):
    import torch
    pb = p.proof_bytes(*p.proof_shape())
    return (torch.full((n, pb), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((n, p.k, 64), 0xEE, dtype=torch.uint8, device="cuda"),
            torch.full((n,), 7, dtype=torch.int32, device="cuda"))          # (an instance no kernel reached keeps the 7)


def _device_prove(p, label, x, s, rnd=None, seed=None, stream_base=0):
    import torch
    n = x.shape[0]
    dx, ds = _dev(x), _dev(s)
    dP, dC, dS = _out(p, n)
    torch.cuda.synchronize()
    if seed is None:
        dr = _dev(rnd)
        torch.cuda.synchronize()
        p.prove_values_batch_device(label, n, dx.data_ptr(), ds.data_ptr(), dr.data_ptr(), dP.data_ptr(), dC.data_ptr(), dS.data_ptr())
    else:
        p.prove_values_batch_seeded_device(label, n, dx.data_ptr(), ds.data_ptr(), seed, stream_base, dP.data_ptr(), dC.data_ptr(), dS.data_ptr())
    p.synchronize()
    torch.cuda.synchronize()
    return dP, dC, dS


@pytest.mark.parametrize("shape", A.SHAPES)
def test_bytes_equal_the_golden_proofs_host_and_device(shape):
    case, coms, proofs, x, s, rnd = _golden_inputs(shape)
    p = _proto(shape)
    assert p.proof_shape() == (case["rounds"], case["nl"], case["nn"])
    got, gcom, st, _ = p.prove_values_batch(case["label"], x, s, rnd)
    assert not st.any(), st.tolist()
    for b in range(len(proofs)):
        assert gcom[b].tobytes() == coms[b].tobytes(), (shape, b, "commitments")
        assert got[b].tobytes() == proofs[b].tobytes(), (shape, b, "proof")
    dP, dC, dS = _device_prove(p, case["label"], x, s, rnd)
    assert dP.cpu().numpy().tobytes() == got.tobytes() and dC.cpu().numpy().tobytes() == gcom.tobytes() and not dS.cpu().numpy().any()


def test_k1_equals_the_reciprocal_prover_from_integers():
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    shape = (1, 4, 4)
    case, coms, proofs, x, s, rnd = _golden_inputs(shape)
    got, gcom, st, _ = _proto(shape).prove_values_batch(case["label"], x, s, rnd)
    r = ReciprocalRangeProofProtocol(4, 4, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0, fb_window_bits=8)
    try:
        assert rnd.shape[1] == 20 + 2 * 4
        rp, rc, rst, _ = r.prove_values_batch(case["label"], x.reshape(-1, 32), s.reshape(-1, 32), rnd)
    finally:
        r.close()
    assert rp.tobytes() == got.tobytes() and rc.tobytes() == gcom.tobytes() and rst.tobytes() == st.tobytes()


@pytest.mark.parametrize("shape", [(2, 4, 4), (7, 3, 4)])
def test_seeded_forms_equal_the_rnd_forms_and_split_calls(shape):
    from bp_pp_amd.range_proof import draw_scalars
    p = _proto(shape)
    case, x, s, _, _ = _rows(shape, ROWS)
    base = 1000
    rnd = draw_scalars(SEED, base, ROWS, p.prove_draws())
    want, wcom, wst, _ = p.prove_values_batch(case["label"], x, s, rnd)
    assert not wst.any()
    got, gcom, st, _ = p.prove_values_batch_seeded(case["label"], x, s, SEED, base)
    assert got.tobytes() == want.tobytes() and gcom.tobytes() == wcom.tobytes() and not st.any()
    dP, dC, dS = _device_prove(p, case["label"], x, s, seed=SEED, stream_base=base)
    assert dP.cpu().numpy().tobytes() == want.tobytes() and dC.cpu().numpy().tobytes() == wcom.tobytes() and not dS.cpu().numpy().any()
    # 33 + 37 with the stream advanced by 33
    a = p.prove_values_batch_seeded(case["label"], x[:33], s[:33], SEED, base)
    b = p.prove_values_batch_seeded(case["label"], x[33:], s[33:], SEED, base + 33)
    assert np.concatenate([a[0], b[0]]).tobytes() == want.tobytes() and np.concatenate([a[1], b[1]]).tobytes() == wcom.tobytes()


@pytest.mark.parametrize("shape,n", [((2, 4, 4), ROWS), ((16, 16, 16), 8)])
def test_round_trip_through_the_device_verifier(shape, n):
    import torch
    p = _proto(shape)
    case, x, s, _, _ = _rows(shape, n)
    dP, dC, dS = _device_prove(p, case["label"], x, s, seed=SEED, stream_base=7)
    assert not dS.cpu().numpy().any()
    rounds, nl, nn = p.proof_shape()

    def verify():
        dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
        dV = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        dR = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        p.verify_batch_device(case["label"], n, dC.data_ptr(), dP.data_ptr(), rounds, nl, nn, dA.data_ptr(), dV.data_ptr(), dR.data_ptr())
        p.synchronize()
        torch.cuda.synchronize()
        return dA.cpu().numpy(), dV.cpu().numpy(), int(dR.cpu()[0])

    acc, vst, rejects = verify()
    assert acc.tolist() == [1] * n and not vst.any() and rejects == 0
    row = n // 2
    dP[row, dP.shape[1] - 1] ^= 1              # the last byte of n: the scalar stays canonical
    torch.cuda.synchronize()
    acc, vst, rejects = verify()
    assert acc.tolist() == [0 if i == row else 1 for i in range(n)] and rejects == 1


@pytest.mark.parametrize("shape", [(3, 4, 4), (16, 16, 16)])
def test_flagged_rows_in_a_batch(shape):
    k, nd, np_ = shape
    p = _proto(shape)
    case, x, s, rnd, _ = _rows(shape, ROWS)
    want, wcom, wst, _ = p.prove_values_batch(case["label"], x, s, rnd)
    assert not wst.any()
    x, s = x.copy(), s.copy()
    flags = {5: ST_OUT_OF_RANGE, 40: ST_BAD_ENCODING, ROWS - 1: ST_BAD_ENCODING}
    x[5, k // 2] = np.frombuffer(AP.be32(np_**nd), np.uint8)               # the middle value one above the range
    x[40, k - 1] = np.frombuffer(AP.be32(A.N), np.uint8)                   # n itself: not canonical
    s[ROWS - 1, 0] = np.frombuffer(AP.be32(A.N + 1), np.uint8)             # the last row (what a short grid drops): a non-canonical s
    got, gcom, st, _ = p.prove_values_batch(case["label"], x, s, rnd)
    dP, dC, dS = _device_prove(p, case["label"], x, s, rnd)
    for proofs, coms, status in ((got, gcom, st), (dP.cpu().numpy(), dC.cpu().numpy(), dS.cpu().numpy())):
        assert status.tolist() == [flags.get(i, 0) for i in range(ROWS)]
        for i in range(ROWS):
            if i in flags:
                assert not proofs[i].any() and not coms[i].any(), i
            else:
                assert proofs[i].tobytes() == want[i].tobytes() and coms[i].tobytes() == wcom[i].tobytes(), i


@pytest.mark.parametrize("shape", [(2, 4, 4), (6, 2, 3)])
def test_ct_prover_changes_no_byte(shape):
    p = _proto(shape)
    case, x, s, rnd, _ = _rows(shape, ROWS)
    want, wcom, wst, _ = p.prove_values_batch(case["label"], x, s, rnd)
    p.set_option("ct_prover", 1)
    try:
        got, gcom, st, _ = p.prove_values_batch(case["label"], x, s, rnd)
        dP, dC, dS = _device_prove(p, case["label"], x, s, rnd)
    finally:
        p.set_option("ct_prover", 0)
    assert got.tobytes() == want.tobytes() and gcom.tobytes() == wcom.tobytes() and st.tobytes() == wst.tobytes()
    assert dP.cpu().numpy().tobytes() == want.tobytes() and dC.cpu().numpy().tobytes() == wcom.tobytes()


def test_refused_shapes_and_null_outputs_launch_nothing():
    from bp_pp_amd import _capi
    L = _capi.lib()
    E = _capi.ERR_INVALID_ARG
    p = _proto((16, 16, 16))                      # 256 generators in g_vec, 32 in h_vec
    ctx = p._w._ctx
    buf = np.zeros(1 << 20, np.uint8)
    q = buf.ctypes.data
    assert L.bppp_reciprocal_agg_prove_draws(16, 16) == 16 + 18 + 17 + 256 == p.prove_draws()
    p.enable_timing(True)
    p.timings()
    try:
        def host(k, nd, np_, x=q, s=q, rnd=q, proofs=q, com=q, n=1):
            return L.bppp_reciprocal_agg_prove_values_batch(ctx, b"x", 1, n, k, nd, np_, x, s, rnd, proofs, com, q)

        def seeded(k, nd, np_, base=0, n=1, seed=SEED):
            return L.bppp_reciprocal_agg_prove_values_batch_seeded_device(ctx, b"x", 1, n, k, nd, np_, q, q, seed, base, q, q, q)

        for f in (host, seeded):
            assert f(0, 16, 16) == E and f(65, 1, 1) == E                 # 1 <= k <= 64
            assert f(16, 17, 16) == E and f(64, 5, 4) == E                # k dim_nd <= |g_vec|
            assert f(2, 23, 16) == E                                      # dim_nd + 10 <= |h_vec|
            assert f(16, 16, 18) == E and f(16, 0, 1) == E and f(16, 16, 0) == E
        # (dim_np^dim_nd > n cannot be reached under dim_nd + 10 <= 32 and dim_np <= dim_nd + 1: 23^22 < 2^100; the rule is tested on a grid
        # in tests/test_agg_prove_emul.py)
        assert host(16, 16, 16, proofs=None) == E and host(16, 16, 16, com=None) == E and host(16, 16, 16, x=None) == E
        assert host(16, 16, 16, s=None) == E and host(16, 16, 16, rnd=None) == E
        assert seeded(16, 16, 16, seed=None) == E
        assert seeded(16, 16, 16, base=(1 << 64) - 1, n=2) == E           # the stream range overflows
        assert L.bppp_reciprocal_agg_prove_values_batch(None, b"x", 1, 1, 2, 4, 4, q, q, q, q, q, q) == E
        assert host(16, 16, 16, n=0) == 0 and seeded(16, 16, 16, n=0) == 0      # the edge itself passes; nothing to do
        assert not any(v["launches"] for v in p.timings(reset=True).values())
    finally:
        p.enable_timing(False)


def test_a_call_in_many_parts_equals_the_one_part_call():
    """"max_batch" bounds the multiplication gates of a part: 1024 / (16 x 16) = 4 instances, so 70 rows run as 18 parts (the last one of
    2) -- host and device forms, the seeded stream carried from part to part."""
    shape = (16, 16, 16)
    p = _proto(shape)
    case, x, s, _, _ = _rows(shape, ROWS)
    want, wcom, wst, _ = p.prove_values_batch_seeded(case["label"], x, s, SEED, 5)
    assert not wst.any()
    before = p.get_option("max_batch")
    p.set_option("max_batch", 1024)
    p.enable_timing(True)
    p.timings()
    try:
        got, gcom, st, _ = p.prove_values_batch_seeded(case["label"], x, s, SEED, 5)
        kt = p.timings()
        assert kt["k_aprove_witness"]["launches"] == 18 and kt["k_aprove_stage_b"]["launches"] == 18 and kt["k_aprove_collect"]["launches"] == 18
        dP, dC, dS = _device_prove(p, case["label"], x, s, seed=SEED, stream_base=5)
    finally:
        p.enable_timing(False)
        p.set_option("max_batch", before)
    assert got.tobytes() == want.tobytes() and gcom.tobytes() == wcom.tobytes() and not st.any()
    assert dP.cpu().numpy().tobytes() == want.tobytes() and dC.cpu().numpy().tobytes() == wcom.tobytes() and not dS.cpu().numpy().any()
