"""GPU tests of the seeded provers (include/bppp.h: "Seeded provers"): the draws made on the device (k_draw_scalars) equal the
library's host draws byte for byte, and every seeded prover equals its `rnd` twin fed with those draws -- u64 host and device forms,
ct_prover, split calls, a one-device group, the generic reciprocal and circuit provers -- with every proof accepted.  A failed
allocation of the draw buffer returns BPPP_ERR_NOMEM and leaves the context usable."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = bytes.fromhex("243f6a8885a308d313198a2e03707344a4093822299f31d0082efa98ec4e6c89")


def _need_gpu():
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")


@pytest.fixture(scope="module")
def proto():
    _need_gpu()
    import workload
    from bp_pp_amd import U64RangeProofProtocol
    g, gv, hv = workload.split_generators(workload.generators())
    p = U64RangeProofProtocol(g, gv, hv, device=0, fb_window_bits=8)
    yield p
    p.close()


def _inputs(n, first=7000):
    import workload
    return np.ascontiguousarray(workload.values(n, first)), np.ascontiguousarray(workload.blindings(n, first))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- the draws
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("k", [1, 52, 532])
def test_device_draws_equal_host_draws(proto, n, k):
    import torch
    from bp_pp_amd import draw_scalars
    base = (1 << 32) - 40                                   # the streams cross 2^32 inside the batch
    want = draw_scalars(SEED, base, n, k)
    guard = 256
    buf = torch.full((n * k * 32 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    proto.draw_scalars_device(SEED, base, n, k, buf.data_ptr())
    proto.synchronize()
    got = buf.cpu().numpy()
    assert (got[:n * k * 32].reshape(n, k, 32) == want).all()
    assert (got[n * k * 32:] == 0xA5).all()                # nothing written past n x k x 32


# ---------------------------------------------------------------- the u64 prover
@pytest.mark.parametrize("n", [1, 700, 1 << 14])
def test_u64_seeded_equals_rnd_twin_and_oracle(proto, oracle_c, n):
    import torch
    import workload
    from bp_pp_amd import draw_scalars
    x, s = _inputs(n)
    base = 1000 + n
    rnd = draw_scalars(SEED, base, n, 52).reshape(n, 52 * 32)
    p0, c0, st0 = proto.prove_batch(x, s, rnd, workload.LABEL)
    p1, c1, st1 = proto.prove_batch_seeded(x, s, SEED, base, workload.LABEL)
    assert not st0.any() and (st0 == st1).all()
    assert (p0 == p1).all() and (c0 == c1).all()
    # the checker's prover on a sample, from the same draws
    idx = sorted({0, n // 2, n - 1})
    op, ov = oracle_c.u64_prove_batch(workload.generators(), workload.LABEL, x[idx], s[idx], rnd[idx], nthreads=len(idx))
    assert (op == p1[idx]).all() and (ov == c1[idx]).all()
    # device form
    dX, dS = _dev(x.view(np.uint8)), _dev(s)
    dP = torch.zeros((n, 928), dtype=torch.uint8, device="cuda")
    dC = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    dSt = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    proto.prove_batch_seeded_device(workload.LABEL, n, dX.data_ptr(), dS.data_ptr(), SEED, base, dP.data_ptr(), dC.data_ptr(), dSt.data_ptr())
    proto.synchronize()
    assert (dP.cpu().numpy() == p1).all() and (dC.cpu().numpy() == c1).all() and not dSt.cpu().numpy().any()
    acc, vst = proto.verify_batch(c1, p1, workload.LABEL)
    assert acc.all() and not vst.any()


@pytest.mark.parametrize("n", [1, 700])
def test_u64_seeded_ct_prover(proto, n):
    import workload
    from bp_pp_amd import draw_scalars
    x, s = _inputs(n, first=8100)
    rnd = draw_scalars(SEED, 77, n, 52).reshape(n, 52 * 32)
    p0, c0, _ = proto.prove_batch(x, s, rnd, workload.LABEL)
    proto.set_option("ct_prover", 1)
    try:
        p1, c1, st1 = proto.prove_batch_seeded(x, s, SEED, 77, workload.LABEL)
    finally:
        proto.set_option("ct_prover", 0)
    assert not st1.any() and (p0 == p1).all() and (c0 == c1).all()


def test_u64_seeded_split_calls_and_group_equal_one_call(proto):
    import workload
    from bp_pp_amd.distributed import U64RangeProofGroup
    n, base = 700, (1 << 40) + 3
    x, s = _inputs(n, first=9300)
    P, V, st = proto.prove_batch_seeded(x, s, SEED, base, workload.LABEL)
    h = n // 2
    Pa, Va, _ = proto.prove_batch_seeded(x[:h], s[:h], SEED, base, workload.LABEL)
    Pb, Vb, _ = proto.prove_batch_seeded(x[h:], s[h:], SEED, base + h, workload.LABEL)
    assert (np.concatenate([Pa, Pb]) == P).all() and (np.concatenate([Va, Vb]) == V).all()
    # another seed or another stream gives other proofs (the draws are what changed)
    Po, _, _ = proto.prove_batch_seeded(x[:4], s[:4], SEED[::-1], base, workload.LABEL)
    Ps, _, _ = proto.prove_batch_seeded(x[:4], s[:4], SEED, base + 1, workload.LABEL)
    assert all((Po[i] != P[i]).any() and (Ps[i] != P[i]).any() for i in range(4))
    g, gv, hv = workload.split_generators(workload.generators())
    grp = U64RangeProofGroup(g, gv, hv, [0], fb_window_bits=8)
    try:
        Pg, Vg, stg = grp.prove_batch_seeded(x, s, SEED, base, workload.LABEL)
        assert (Pg == P).all() and (Vg == V).all() and (stg == st).all()
    finally:
        grp.close()


def test_u64_seeded_bad_arguments(proto):
    import workload
    from bp_pp_amd import BpppError, _capi
    x, s = _inputs(3)
    with pytest.raises(ValueError):
        proto.prove_batch_seeded(x, s, SEED, (1 << 64) - 2, workload.LABEL)
    with pytest.raises(ValueError):
        proto.prove_batch_seeded(x, s, SEED[:16], 0, workload.LABEL)
    L = _capi.lib()
    out = np.zeros((3, 928), np.uint8)
    com = np.zeros((3, 64), np.uint8)
    rc = L.bppp_u64_prove_batch_seeded(proto._ctx, workload.LABEL, len(workload.LABEL), 3, x.ctypes.data, s.ctypes.data, SEED,
                                       (1 << 64) - 2, out.ctypes.data, com.ctypes.data, None)
    assert rc == _capi.ERR_INVALID_ARG
    rc = L.bppp_u64_prove_batch_seeded(proto._ctx, workload.LABEL, len(workload.LABEL), 3, x.ctypes.data, s.ctypes.data, None, 0,
                                       out.ctypes.data, com.ctypes.data, None)
    assert rc == _capi.ERR_INVALID_ARG
    assert isinstance(BpppError(rc), RuntimeError)


def test_draw_buffer_allocation_failure_leaves_the_context_usable():
    _need_gpu()
    import torch
    import workload
    from bp_pp_amd import BpppError, U64RangeProofProtocol, _capi
    g, gv, hv = workload.split_generators(workload.generators())
    p = U64RangeProofProtocol(g, gv, hv, device=0, fb_window_bits=8)
    try:
        n = 65
        x, s = _inputs(n, first=9900)
        dX, dS = _dev(x.view(np.uint8)), _dev(s)
        dP = torch.zeros((n, 928), dtype=torch.uint8, device="cuda")
        dC = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        before = p.device_bytes()
        p.set_option("inject_alloc_fault", 1)             # the next device allocation of the context: the draw buffer
        with pytest.raises(BpppError) as e:
            p.prove_batch_seeded_device(workload.LABEL, n, dX.data_ptr(), dS.data_ptr(), SEED, 5, dP.data_ptr(), dC.data_ptr())
        assert e.value.code == _capi.ERR_NOMEM
        assert p.device_bytes() == before
        p.prove_batch_seeded_device(workload.LABEL, n, dX.data_ptr(), dS.data_ptr(), SEED, 5, dP.data_ptr(), dC.data_ptr())
        p.synchronize()
        P, V, st = p.prove_batch_seeded(x, s, SEED, 5, workload.LABEL)
        assert not st.any() and (dP.cpu().numpy() == P).all() and (dC.cpu().numpy() == V).all()
        acc, _ = p.verify_batch(V, P, workload.LABEL)
        assert acc.all()
    finally:
        p.close()


# ---------------------------------------------------------------- the generic provers
@pytest.mark.parametrize("nd,npp,B", [(8, 4, 5), (16, 16, 5), (32, 16, 5), (256, 16, 3)])
def test_reciprocal_seeded_equals_rnd_twin(nd, npp, B):
    _need_gpu()
    import recip_cases
    from bp_pp_amd import draw_scalars
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    case = recip_cases.make(nd, npp, B, n_oracle=0)
    proto = ReciprocalRangeProofProtocol(nd, npp, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0,
                                         fb_window_bits=8 if nd > 64 else 16)
    try:
        com, cst = proto.commit_value_batch(case["x"], case["s"])
        assert not cst.any()
        base = 31 * nd
        rnd = draw_scalars(SEED, base, B, 20 + 2 * nd)
        args = (case["x"], case["s"], case["digits"], case["m"])
        p0, st0, shape0 = proto.prove_batch(case["label"], com, *args, rnd)
        p1, st1, shape1 = proto.prove_batch_seeded(case["label"], com, *args, SEED, base)
        assert shape0 == shape1 and not st0.any() and not st1.any()
        assert (p0 == p1).all()
        acc, vst = proto.verify_batch(case["label"], com, p1, *shape1)
        assert acc.all() and not vst.any()
        p2, _, _ = proto.prove_batch_seeded(case["label"], com, *args, SEED, base + 1)
        assert all((p2[i] != p1[i]).any() for i in range(B))
    finally:
        proto.close()


def test_reciprocal_seeded_refuses_what_its_twin_refuses():
    """dim_np > dim_nd + 1 (e.g. (8, 16)) is outside the prover's shapes: both forms return BPPP_ERR_INVALID_ARG."""
    _need_gpu()
    import recip_cases
    from bp_pp_amd import BpppError, _capi
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    case = recip_cases.make(8, 4, 2, n_oracle=0)
    proto = ReciprocalRangeProofProtocol(8, 16, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0, fb_window_bits=16)
    try:
        com = np.zeros((2, 64), np.uint8)
        m = np.zeros((2, 16, 32), np.uint8)
        args = (case["x"], case["s"], case["digits"], m)
        for call in (lambda: proto.prove_batch(case["label"], com, *args, np.zeros((2, 36, 32), np.uint8)),
                     lambda: proto.prove_batch_seeded(case["label"], com, *args, SEED, 0)):
            with pytest.raises(BpppError) as e:
                call()
            assert e.value.code == _capi.ERR_INVALID_ARG
    finally:
        proto.close()


def test_circuit_seeded_equals_rnd_twin():
    _need_gpu()
    import circuit_cases
    from bp_pp_amd import draw_scalars
    from bp_pp_amd.wnla import ArithmeticCircuit
    case = circuit_cases.make("mixed_k2", 3)
    part = lambda typ, j: (None if case["part"][typ][j] < 0 else int(case["part"][typ][j]))
    arr = lambda b: np.frombuffer(b, np.uint8).reshape(-1, 32)
    circ = ArithmeticCircuit(case["nm"], case["no"], case["k"], case["nv"], case["g"], case["gv"], case["hv"], arr(case["Wm_bytes"]),
                             arr(case["Wl_bytes"]), arr(case["am_bytes"]), arr(case["al_bytes"]), case["f_l"], case["f_m"], case["gv_"],
                             case["hv_"], part, device=0, fb_window_bits=16)
    try:
        B = 3
        args = (case["v_bytes"], case["s_v"], case["wl_bytes"], case["wr_bytes"], case["wo_bytes"])
        rnd = draw_scalars(SEED, 900, B, 18 + case["nv"] + case["nm"])
        p0, st0, shape0 = circ.prove_batch(case["label"], case["commitments"], *args, rnd)
        p1, st1, shape1 = circ.prove_batch_seeded(case["label"], case["commitments"], *args, SEED, 900)
        assert shape0 == shape1 and not st0.any() and not st1.any()
        assert (p0 == p1).all()
        acc, vst = circ.verify_batch(case["label"], case["commitments"], p1, *shape1)
        assert acc.all() and not vst.any()
    finally:
        circ.close()
