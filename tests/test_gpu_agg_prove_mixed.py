"""The aggregated reciprocal range proof PROVER for MIXED value counts on the GPU (bppp_reciprocal_agg_prove_values_batch_mixed*;
csrc/agg_prove_mixed_core.h, k_aggprove_mixed.hip): instance i has ks[i] values, every buffer laid out by k_max.  Every comparison is
bit-exact.

The expected bytes are the oracle's pool proofs for every value count on the k_max context's generators (tests/golden/
agg_mixed_cases.json); tests/agg_prove_mixed_cases.py rebuilds the inputs the oracle was fed and lays them out by k_max with 0xFF in every
unused x, s and rnd slot, so every test here also shows that nothing unused is read.  Context shapes (k_max, nd, np) and value counts:
    (3, 4, 4)     1..3           the smallest
    (7, 3, 4)     1..7           nm = 21 padded to 32
    (6, 2, 3)     1..6           np = nd + 1
    (16, 16, 16)  1, 9, 15, 16   sixteen u64 values, one pool proof per count (8 rows)
Batches of 70 rows cross a wavefront boundary with a ragged last block."""
import numpy as np
import pytest

import agg_cases as A
import agg_mixed_cases as M
import agg_prove_cases as AP
import agg_prove_mixed_cases as PM

pytestmark = pytest.mark.gpu

SEED = bytes.fromhex("243f6a8885a308d313198a2e03707344a4093822299f31d0082efa98ec4e6c89")
ST_BAD_ENCODING, ST_OUT_OF_RANGE = 1, 4
ROWS = 70
SMALL = [s for s in M.CONTEXTS if s != (16, 16, 16)]
NEW_KERNELS = ["k_aprove_mixed_witness", "k_aprove_mixed_commit", "k_aprove_mixed_poles", "k_aprove_mixed_stage_a", "k_aprove_mixed_stage_b",
               "k_aprove_mixed_collect", "k_aprove_mixed_tail", "k_aprove_mixed_assemble"]
_made = {}


def _proto(shape, k=None):
    """The protocol object of k values on the context of `shape` (k = None: k_max, the mixed calls' object)."""
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol
    k = shape[0] if k is None else k
    if (shape, k) not in _made:
        case = M.setup_on(M.load_pool(shape)[0], k)
        _made[(shape, k)] = AggregatedReciprocalRangeProofProtocol(k, shape[1], shape[2], case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"],
                                                                   device=0, fb_window_bits=8)
    return _made[(shape, k)]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for p in _made.values():
        p.close()
    _made.clear()


def _rows(shape):
    return 8 if shape == (16, 16, 16) else ROWS


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _device_prove(p, label, ks, x, s, rnd=None, seed=None, stream_base=0):
    import torch
    n = len(ks)
    dk, dx, ds = _dev(np.asarray(ks, np.uint8)), _dev(x), _dev(s)
    pb = p.proof_bytes(*p.proof_shape())
    dP = torch.full((n, pb), 0xEE, dtype=torch.uint8, device="cuda")
    dC = torch.full((n, p.k, 64), 0xEE, dtype=torch.uint8, device="cuda")
    dS = torch.full((n,), 7, dtype=torch.int32, device="cuda")          # (an instance no kernel reached keeps the 7)
    torch.cuda.synchronize()
    if seed is None:
        dr = _dev(rnd)
        torch.cuda.synchronize()
        p.prove_values_batch_mixed_device(label, n, dk.data_ptr(), dx.data_ptr(), ds.data_ptr(), dr.data_ptr(), dP.data_ptr(), dC.data_ptr(),
                                          dS.data_ptr())
    else:
        p.prove_values_batch_mixed_seeded_device(label, n, dk.data_ptr(), dx.data_ptr(), ds.data_ptr(), seed, stream_base, dP.data_ptr(),
                                                 dC.data_ptr(), dS.data_ptr())
    p.synchronize()
    torch.cuda.synchronize()
    return dP, dC, dS, dk


def _same(got, want):
    return np.asarray(got).tobytes() == np.asarray(want).tobytes()


@pytest.mark.parametrize("shape", list(M.CONTEXTS))
def test_bytes_equal_the_golden_pool_host_and_device(shape):
    p = _proto(shape)
    case_max, _ = M.load_pool(shape)
    assert p.proof_shape() == (case_max["rounds"], case_max["nl"], case_max["nn"]) and p.prove_draws() == PM.draws(*shape[:2])
    ks = PM.cycle(shape, _rows(shape))
    x, s, rnd, C, Q = PM.build(shape, ks)                                # (0xFF in every unused slot: not read, nothing flagged)
    got, gcom, st, _ = p.prove_values_batch_mixed(case_max["label"], ks, x, s, rnd)
    assert not st.any(), st.tolist()
    for t, k in enumerate(ks):
        pb = M.setup_on(case_max, k)["proof_bytes"]
        assert _same(gcom[t, :k], C[t, :k]) and not gcom[t, k:].any(), (shape, t, k, "commitments")
        assert _same(got[t, :pb], Q[t, :pb]) and not got[t, pb:].any(), (shape, t, k, "proof")
    dP, dC, dS, _ = _device_prove(p, case_max["label"], ks, x, s, rnd)
    assert _same(dP.cpu().numpy(), Q) and _same(dC.cpu().numpy(), C) and not dS.cpu().numpy().any()


def test_every_count_equals_the_uniform_prover_on_the_same_context():
    shape = (7, 3, 4)
    p = _proto(shape)
    case_max, _ = M.load_pool(shape)
    ks = PM.cycle(shape, ROWS)
    x, s, rnd, _, _ = PM.build(shape, ks)
    got, gcom, st, _ = p.prove_values_batch_mixed(case_max["label"], ks, x, s, rnd)
    assert not st.any()
    ks = np.asarray(ks)
    for k in M.CONTEXTS[shape]:
        idx = np.flatnonzero(ks == k)
        u = _proto(shape, k)
        D = u.prove_draws()
        up, uc, ust, _ = u.prove_values_batch(case_max["label"], x[idx, :k], s[idx, :k], rnd[idx, :D])
        assert not ust.any()
        pb = up.shape[1]
        assert _same(got[idx, :pb], up) and not got[idx, pb:].any(), k
        assert _same(gcom[idx, :k], uc) and not gcom[idx, k:].any(), k


def test_a_wavefront_of_one_count_next_to_a_wavefront_of_all_counts():
    shape = (7, 3, 4)
    p = _proto(shape)
    case_max, _ = M.load_pool(shape)
    ks = [5] * 64 + PM.cycle(shape, 64) + [1] * 6
    x, s, rnd, C, Q = PM.build(shape, ks)
    dP, dC, dS, _ = _device_prove(p, case_max["label"], ks, x, s, rnd)
    assert not dS.cpu().numpy().any() and _same(dP.cpu().numpy(), Q) and _same(dC.cpu().numpy(), C)


@pytest.mark.parametrize("shape", [(3, 4, 4), (7, 3, 4)])
def test_seeded_forms_equal_the_rnd_forms_and_split_calls(shape):
    from bp_pp_amd.range_proof import draw_scalars
    p = _proto(shape)
    case_max, _ = M.load_pool(shape)
    ks = PM.cycle(shape, ROWS)
    x, s, _, _, _ = PM.build(shape, ks)
    base = 1000
    rnd = draw_scalars(SEED, base, ROWS, p.prove_draws())
    want, wcom, wst, _ = p.prove_values_batch_mixed(case_max["label"], ks, x, s, rnd)
    assert not wst.any() and want.any(axis=1).all()
    got, gcom, st, _ = p.prove_values_batch_mixed_seeded(case_max["label"], ks, x, s, SEED, base)
    assert _same(got, want) and _same(gcom, wcom) and not st.any()
    dP, dC, dS, _ = _device_prove(p, case_max["label"], ks, x, s, seed=SEED, stream_base=base)
    assert _same(dP.cpu().numpy(), want) and _same(dC.cpu().numpy(), wcom) and not dS.cpu().numpy().any()
    # 33 + 37 with the stream advanced by 33
    a = p.prove_values_batch_mixed_seeded(case_max["label"], ks[:33], x[:33], s[:33], SEED, base)
    b = p.prove_values_batch_mixed_seeded(case_max["label"], ks[33:], x[33:], s[33:], SEED, base + 33)
    assert _same(np.concatenate([a[0], b[0]]), want) and _same(np.concatenate([a[1], b[1]]), wcom)


@pytest.mark.parametrize("shape", [(7, 3, 4), (16, 16, 16)])
def test_round_trip_through_the_mixed_device_verifier(shape):
    import torch
    p = _proto(shape)
    case_max, _ = M.load_pool(shape)
    n = _rows(shape)
    ks = PM.cycle(shape, n)
    x, s, _, _, _ = PM.build(shape, ks)
    dP, dC, dS, dk = _device_prove(p, case_max["label"], ks, x, s, seed=SEED, stream_base=7)
    assert not dS.cpu().numpy().any()
    rounds, nl, nn = p.proof_shape()

    def verify():
        dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
        dV = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        dR = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        p.verify_batch_mixed_device(case_max["label"], n, dk.data_ptr(), dC.data_ptr(), dP.data_ptr(), rounds, nl, nn, dA.data_ptr(),
                                    dV.data_ptr(), dR.data_ptr())
        p.synchronize()
        torch.cuda.synchronize()
        return dA.cpu().numpy(), dV.cpu().numpy(), int(dR.cpu()[0])

    acc, vst, rejects = verify()                                          # the prover's outputs, unmodified
    assert acc.tolist() == [1] * n and not vst.any() and rejects == 0
    row = n // 2
    last = M.setup_on(case_max, ks[row])["proof_bytes"] - 1               # the last byte of this row's n: the scalar stays canonical
    dP[row, last] ^= 1
    torch.cuda.synchronize()
    acc, vst, rejects = verify()
    assert acc.tolist() == [0 if i == row else 1 for i in range(n)] and rejects == 1


@pytest.mark.parametrize("shape", [(3, 4, 4), (7, 3, 4)])
def test_flagged_rows_in_a_batch(shape):
    k_max, nd, np_ = shape
    p = _proto(shape)
    case_max, _ = M.load_pool(shape)
    ks = PM.cycle(shape, ROWS)
    x, s, rnd, C, Q = PM.build(shape, ks)
    x, s = x.copy(), s.copy()
    last = ROWS - 1
    flags = {5: ST_OUT_OF_RANGE, 40: ST_BAD_ENCODING, last: ST_BAD_ENCODING}
    x[5, ks[5] // 2] = np.frombuffer(AP.be32(np_**nd), np.uint8)           # a used value one above the range
    x[40, ks[40] - 1] = np.frombuffer(AP.be32(A.N), np.uint8)              # the last used x: n itself, not canonical
    s[last, 0] = np.frombuffer(AP.be32(A.N + 1), np.uint8)                 # the last row (what a short grid drops): a non-canonical s
    got, gcom, st, _ = p.prove_values_batch_mixed(case_max["label"], ks, x, s, rnd)
    dP, dC, dS, _ = _device_prove(p, case_max["label"], ks, x, s, rnd)
    # the device form cannot refuse a count: 0 and k_max + 1 are flagged where they are read
    ks_bad = list(ks)
    ks_bad[11], ks_bad[64] = 0, k_max + 1
    bP, bC, bS, _ = _device_prove(p, case_max["label"], ks_bad, x, s, rnd)
    bad_flags = dict(flags)
    bad_flags.update({11: ST_BAD_ENCODING, 64: ST_BAD_ENCODING})
    for proofs, coms, status, fl in ((got, gcom, st, flags), (dP.cpu().numpy(), dC.cpu().numpy(), dS.cpu().numpy(), flags),
                                     (bP.cpu().numpy(), bC.cpu().numpy(), bS.cpu().numpy(), bad_flags)):
        assert status.tolist() == [fl.get(i, 0) for i in range(ROWS)]
        for i in range(ROWS):
            if i in fl:
                assert not proofs[i].any() and not coms[i].any(), i
            else:
                assert _same(proofs[i], Q[i]) and _same(coms[i], C[i]), i
    with pytest.raises(Exception):                                        # the host form reads ks and refuses the call
        p.prove_values_batch_mixed(case_max["label"], ks_bad, x, s, rnd)


@pytest.mark.parametrize("shape", [(3, 4, 4), (6, 2, 3)])
def test_ct_prover_changes_no_byte(shape):
    p = _proto(shape)
    case_max, _ = M.load_pool(shape)
    ks = PM.cycle(shape, ROWS)
    x, s, rnd, C, Q = PM.build(shape, ks)
    p.set_option("ct_prover", 1)
    try:
        got, gcom, st, _ = p.prove_values_batch_mixed(case_max["label"], ks, x, s, rnd)
        dP, dC, dS, _ = _device_prove(p, case_max["label"], ks, x, s, rnd)
    finally:
        p.set_option("ct_prover", 0)
    assert _same(got, Q) and _same(gcom, C) and not st.any()
    assert _same(dP.cpu().numpy(), Q) and _same(dC.cpu().numpy(), C) and not dS.cpu().numpy().any()


def test_a_call_in_parts_equals_the_one_part_call():
    """"max_batch" bounds the multiplication gates of a part by k_max dim_nd: 1024 / (16 x 16) = 4 instances, so 8 rows run as 2 parts,
    each on its own slice of ks -- host and device forms, the seeded stream carried from part to part."""
    shape = (16, 16, 16)
    p = _proto(shape)
    case_max, _ = M.load_pool(shape)
    ks = PM.cycle(shape, 8, start=1)                                      # (the parts' slices of ks differ from the whole's start)
    x, s, _, _, _ = PM.build(shape, ks)
    want, wcom, wst, _ = p.prove_values_batch_mixed_seeded(case_max["label"], ks, x, s, SEED, 5)
    assert not wst.any() and want.any(axis=1).all()
    before = p.get_option("max_batch")
    p.set_option("max_batch", 1024)
    p.enable_timing(True)
    p.timings()
    try:
        got, gcom, st, _ = p.prove_values_batch_mixed_seeded(case_max["label"], ks, x, s, SEED, 5)
        kt = p.timings()
        assert [kt[name]["launches"] for name in NEW_KERNELS] == [2] * len(NEW_KERNELS), kt
        assert not kt["k_aprove_witness"]["launches"] and not kt["k_aprove_stage_b"]["launches"]      # (nothing of the uniform chain's own)
        dP, dC, dS, _ = _device_prove(p, case_max["label"], ks, x, s, seed=SEED, stream_base=5)
    finally:
        p.enable_timing(False)
        p.set_option("max_batch", before)
    assert _same(got, want) and _same(gcom, wcom) and not st.any()
    assert _same(dP.cpu().numpy(), want) and _same(dC.cpu().numpy(), wcom) and not dS.cpu().numpy().any()


def test_refused_arguments_launch_nothing():
    from bp_pp_amd import _capi
    L = _capi.lib()
    E = _capi.ERR_INVALID_ARG
    p = _proto((16, 16, 16))                      # 256 generators in g_vec, 32 in h_vec
    ctx = p._w._ctx
    buf = np.ones(1 << 20, np.uint8)              # (as ks: all ones)
    q = buf.ctypes.data
    p.enable_timing(True)
    p.timings()
    try:
        def host(k, nd, np_, ks=q, x=q, s=q, rnd=q, proofs=q, com=q, n=1):
            return L.bppp_reciprocal_agg_prove_values_batch_mixed(ctx, b"x", 1, n, k, ks, nd, np_, x, s, rnd, proofs, com, q)

        def seeded(k, nd, np_, ks=q, base=0, n=1, seed=SEED):
            return L.bppp_reciprocal_agg_prove_values_batch_mixed_seeded_device(ctx, b"x", 1, n, k, ks, nd, np_, q, q, seed, base, q, q, q)

        for f in (host, seeded):
            assert f(0, 16, 16) == E and f(65, 1, 1) == E                 # 1 <= k_max <= 64
            assert f(16, 17, 16) == E and f(64, 5, 4) == E                # k_max dim_nd <= |g_vec|
            assert f(2, 23, 16) == E                                      # dim_nd + 10 <= |h_vec|
            assert f(16, 16, 18) == E and f(16, 0, 1) == E and f(16, 16, 0) == E
            assert f(16, 16, 16, ks=None) == E and f(16, 16, 16, ks=None, n=0) == E
        assert host(16, 16, 16, proofs=None) == E and host(16, 16, 16, com=None) == E and host(16, 16, 16, x=None) == E
        assert host(16, 16, 16, s=None) == E and host(16, 16, 16, rnd=None) == E
        for bad in ([0, 1, 1], [1, 17, 1], [1, 1, 17]):                   # the host form reads ks: first, middle, last
            arr = np.asarray(bad, np.uint8)
            assert host(16, 16, 16, ks=arr.ctypes.data, n=3) == E, bad
        assert seeded(16, 16, 16, seed=None) == E
        assert seeded(16, 16, 16, base=(1 << 64) - 1, n=2) == E           # the stream range overflows
        assert host(16, 16, 16, n=0) == 0 and seeded(16, 16, 16, n=0) == 0      # the edge itself passes; nothing to do
        assert not any(v["launches"] for v in p.timings(reset=True).values())
    finally:
        p.enable_timing(False)
