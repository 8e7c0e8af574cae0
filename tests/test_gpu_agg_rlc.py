"""The RLC mode of the aggregated reciprocal range proof verifier on the GPU (bppp_reciprocal_agg_verify_batch_rlc[_sec1][_device]),
after tests/test_gpu_generic_rlc.py: accept bits and statuses equal the exact call's and the oracle's golden verdicts
(agg_golden.batch) at every batch size around the chunk of 8 -- 1 and 7 (no complete chunk: the exact final sum, reported as (0, 0)),
8, 9 and the 70 rows with their ragged tail -- with the bucket stage over superchunks of 64 and without it, in parts of "max_batch",
after an allocation failure, over the wire form, and at k = 1.

"max_batch" takes no value below 1024, so the call in parts is 1024 + 6 rows with "max_batch" = 1024: the second part has fewer
than 8 instances and runs the exact sum, while the call reports the first part's chunk of 8."""
import numpy as np
import pytest

import agg_cases as A
import agg_golden
from test_gpu_agg_sec1 import PARTS_ROWS, device_call, make, shape_of, wire_batch

pytestmark = pytest.mark.gpu

SHAPES = [(2, 4, 4), (6, 2, 3), (16, 16, 16)]
SIZES = (1, 7, 8, 9, 70)
CHUNK = 8
SUPER = 64                                   # the smallest superchunk "rlc_superchunk" takes
N_SUPER = 2 * SUPER + 3
SEEDS = (bytes(range(7, 39)), bytes(range(200, 232)))
RLC_KERNELS = ("k_wnla_rlc_lhs", "k_wnla_rlc_chunk", "k_wnla_rlc_check", "k_bkt_prepare", "k_bkt_accumulate", "k_bkt_scalars", "k_bkt_check")


@pytest.fixture(scope="module")
def verifiers():
    """Per shape one context that chooses its superchunk by itself; "fixed": one whose "rlc_superchunk" the tests set (the option cannot
    be put back to automatic); "k1": the (1, 4, 4) shape."""
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    made = {}
    try:
        for shape in SHAPES:
            made[shape] = make(shape)
        made["fixed"] = make((2, 4, 4))
        made["k1"] = make((1, 4, 4))
        yield made
    finally:
        for v in made.values():
            v.close()


def _used(v):
    return v.get_option("last_rlc_superchunk"), v.get_option("last_rlc_chunk")


def _check(v, case, Cn, Qn, exp_acc, exp_flag, used, tag):
    """Both seeds through the host and the device RLC form, the exact call between them: byte-equal, and the expected verdicts."""
    args = (case["label"], Cn, Qn, *shape_of(case))
    acc_e, st_e = v.verify_batch(*args)
    assert (acc_e == exp_acc).all() and ((st_e != 0) == exp_flag).all(), (tag, "exact vs expected", acc_e.tolist(), st_e.tolist())
    rej_e = int((acc_e == 0).sum())
    for seed in SEEDS:
        acc, st = v.verify_batch_rlc(*args, seed)
        assert _used(v) == used, (tag, _used(v))
        assert acc.tobytes() == acc_e.tobytes() and st.tobytes() == st_e.tobytes(), (tag, "rlc host", acc.tolist(), st.tolist())
        dacc, dst, rej = device_call(v, case, Cn, Qn, "verify_batch_rlc_device", seed)
        assert _used(v) == used, (tag, _used(v))
        assert dacc.tobytes() == acc_e.tobytes() and dst.tobytes() == st_e.tobytes(), (tag, "rlc device", dacc.tolist(), dst.tolist())
        assert rej == rej_e, (tag, rej, rej_e)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", SHAPES)
def test_rlc_equals_exact_and_the_golden_verdicts_around_the_chunk_size(verifiers, shape, n):
    """The automatic superchunk is 256 at these sizes: one ragged superchunk in front of the chunks of 8."""
    case, Cn, Qn, exp_acc, exp_flag, _ = agg_golden.batch(shape)
    used = (256, CHUNK) if n >= CHUNK else (0, 0)
    _check(verifiers[shape], case, np.ascontiguousarray(Cn[:n]), np.ascontiguousarray(Qn[:n]), exp_acc[:n], exp_flag[:n], used, (shape, n))


def _valid_tiled(n):
    case, Cn, Qn, exp_acc, _, _ = agg_golden.batch((2, 4, 4))
    idx = np.flatnonzero(exp_acc == 1)[np.arange(n) % int(exp_acc.sum())]
    return case, np.ascontiguousarray(Cn[idx]), np.ascontiguousarray(Qn[idx])


def _tamper(Q, i):
    """Well-formed and wrong: a bit flipped in the last proof scalar (never its top byte: the value stays below the group order)."""
    Q[i, Q.shape[1] - 32 + 17] ^= 0x10


def _malform(Q, i):
    """A bad encoding: the first round point off the curve."""
    Q[i, 256 + 63] ^= 1


def test_rlc_bucket_stage_on_two_superchunks_and_a_ragged_one_and_off(verifiers):
    v = verifiers["fixed"]
    n = N_SUPER
    case, Cn, Q0 = _valid_tiled(n)
    batches = [("all valid", Q0, [], [])]
    Q = Q0.copy()
    _tamper(Q, 11)                                # superchunk 0 fails, 1 and 2 pass
    batches.append(("one bad proof in superchunk 0", Q, [11], []))
    Q = Q0.copy()
    _tamper(Q, SUPER + 9)
    _tamper(Q, SUPER + 14)                        # two of one chunk of superchunk 1
    _malform(Q, 20)                               # superchunk 0: a flagged instance has weight zero
    _tamper(Q, n - 1)                             # the last row of the ragged superchunk
    batches.append(("two bad in one chunk of superchunk 1, a bad encoding in 0, the last row", Q, [SUPER + 9, SUPER + 14, n - 1], [20]))
    Q = Q0.copy()
    for i in range(n):
        _tamper(Q, i)
    batches.append(("all invalid", Q, list(range(n)), []))
    for M in (SUPER, 0):
        v.set_option("rlc_superchunk", M)
        for what, Q, bad, flagged in batches:
            exp_acc, exp_flag = np.ones(n, np.uint8), np.zeros(n, bool)
            exp_acc[bad + flagged], exp_flag[flagged] = 0, True
            _check(v, case, Cn, Q, exp_acc, exp_flag, (M, CHUNK), (what, M))


def test_rlc_kernels_show_in_the_timings(verifiers):
    """What shows that the chunk stage ran, rather than everything falling through to the exact sums."""
    shape = (2, 4, 4)
    v = verifiers[shape]
    case, Cn, Qn, exp_acc, exp_flag, _ = agg_golden.batch(shape)
    v.enable_timing(True)
    try:
        v.timings()                                  # (reset)
        acc, st, _ = device_call(v, case, Cn, Qn, "verify_batch_rlc_device", SEEDS[0])
        kt = v.timings()
        acc_e, st_e, _ = device_call(v, case, Cn, Qn, "verify_batch_device")
        ke = v.timings()
    finally:
        v.enable_timing(False)
    assert (acc == exp_acc).all() and ((st != 0) == exp_flag).all() and acc.tobytes() == acc_e.tobytes() and st.tobytes() == st_e.tobytes()
    for name in RLC_KERNELS:
        assert kt[name]["launches"] == 1, (name, kt.get(name))
        assert name not in ke or ke[name]["launches"] == 0, (name, ke.get(name))
    assert kt["k_wnla_msm"]["launches"] == 2 and kt["k_agg_phase1"]["launches"] == 1
    assert ke["k_wnla_msm"]["launches"] == 1 and ke["k_agg_phase1"]["launches"] == 1


def test_rlc_in_parts_of_max_batch(verifiers):
    shape = (2, 4, 4)
    v = verifiers[shape]
    case, Cn, Qn, exp_acc, exp_flag, _ = agg_golden.batch(shape)
    idx = np.arange(PARTS_ROWS) % A.ROWS
    idx[-1] = A.ROWS - 1                              # the call's last row: a corrupted one, in the part that runs the exact sum
    before = v.get_option("max_batch")
    v.set_option("max_batch", 1024)
    try:
        _check(v, case, np.ascontiguousarray(Cn[idx]), np.ascontiguousarray(Qn[idx]), exp_acc[idx], exp_flag[idx], (256, CHUNK), "parts")
    finally:
        v.set_option("max_batch", before)


@pytest.mark.parametrize("form", ["host", "device"])
def test_rlc_allocation_failure_is_nomem_and_the_context_recovers(form):
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    from bp_pp_amd._capi import ERR_NOMEM, BpppError
    shape = (2, 4, 4)
    case, Cn, Qn, exp_acc, exp_flag, _ = agg_golden.batch(shape)
    v = make(shape)
    try:
        run = (lambda: v.verify_batch_rlc(case["label"], Cn, Qn, *shape_of(case), SEEDS[0])) if form == "host" else \
            (lambda: device_call(v, case, Cn, Qn, "verify_batch_rlc_device", SEEDS[0])[:2])
        acc, st = run()
        assert _used(v) == (256, CHUNK)
        big = np.arange(3 * A.ROWS) % A.ROWS          # larger than any call so far: the workspace grows
        v.set_option("inject_alloc_fault", 1)
        with pytest.raises(BpppError) as e:
            if form == "host":
                v.verify_batch_rlc(case["label"], Cn[big], Qn[big], *shape_of(case), SEEDS[0])
            else:
                device_call(v, case, Cn[big], Qn[big], "verify_batch_rlc_device", SEEDS[0])
        assert e.value.code == ERR_NOMEM
        assert _used(v) == (0, 0)                     # nothing stale after the failure
        v.set_option("inject_alloc_fault", 0)
        acc, st = run()                               # the next call is served
        assert (acc == exp_acc).all() and ((st != 0) == exp_flag).all() and _used(v) == (256, CHUNK)
    finally:
        v.close()


def test_rlc_over_the_wire_equals_the_exact_wire_call(verifiers):
    """The (2, 4, 4) wire batch of tests/test_gpu_agg_sec1.py, undecodable rows included: a flagged instance is in no weighted sum."""
    shape = (2, 4, 4)
    v = verifiers[shape]
    case, C33, Q33, exp_acc, exp_flag = wire_batch(shape)
    acc_e, st_e = v.verify_batch_sec1(case["label"], C33, Q33, *shape_of(case))
    assert (acc_e == exp_acc).all() and ((st_e != 0) == exp_flag).all()
    for seed in SEEDS:
        acc, st = v.verify_batch_rlc_sec1(case["label"], C33, Q33, *shape_of(case), seed)
        assert _used(v) == (256, CHUNK)
        dacc, dst, rej = device_call(v, case, C33, Q33, "verify_batch_rlc_sec1_device", seed)
        assert acc.tobytes() == acc_e.tobytes() == dacc.tobytes() and st.tobytes() == st_e.tobytes() == dst.tobytes()
        assert rej == int((exp_acc == 0).sum())


def test_k1_equals_the_reciprocal_rlc_verifier_on_the_same_bytes_and_seed(verifiers):
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    shape = (1, 4, 4)
    case, Cn, Qn, exp_acc, exp_flag, _ = agg_golden.batch(shape)
    r = ReciprocalRangeProofProtocol(4, 4, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0, fb_window_bits=8)
    try:
        racc, rst = r.verify_batch_rlc(case["label"], Cn.reshape(-1, 64), Qn, *shape_of(case), SEEDS[0])
    finally:
        r.close()
    v = verifiers["k1"]
    acc, st = v.verify_batch_rlc(case["label"], Cn, Qn, *shape_of(case), SEEDS[0])
    dacc, dst, rej = device_call(v, case, Cn, Qn, "verify_batch_rlc_device", SEEDS[0])
    assert acc.tobytes() == racc.tobytes() == dacc.tobytes() and st.tobytes() == rst.tobytes() == dst.tobytes()
    assert rej == int((racc == 0).sum())
    assert (acc == exp_acc).all() and ((st != 0) == exp_flag).all()
    assert v._w.generic_form()["protocol"] == "reciprocal"


def test_a_null_seed_and_a_label_merlin_cannot_frame_are_refused_on_a_live_context(verifiers):
    """The C symbols themselves (the Python mirror refuses a seed of None before the call): with a context, buffers and sizes that
    pass every other check, a NULL seed alone and a label of 2^32 bytes alone are BPPP_ERR_INVALID_ARG, at k > 1 and at the k = 1
    forward; the same call with a seed and the label's real length is served."""
    import ctypes as C
    import torch
    from bp_pp_amd import _capi
    L, E = _capi.lib(), _capi.ERR_INVALID_ARG
    too_long = C.c_size_t(1 << 32)
    for key, shape in (((2, 4, 4), (2, 4, 4)), ("k1", (1, 4, 4))):
        v = verifiers[key]
        ctx = v._w._ctx
        case, C33, Q33, exp_acc, _ = wire_batch(shape)
        _, Cn, Qn, _, _, _ = agg_golden.batch(shape)
        n, k, label = A.ROWS, shape[0], case["label"]
        acc, st = np.zeros(n, np.uint8), np.zeros(n, np.int32)
        dA, dS = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        for suffix, com, pr in (("", Cn, Qn), ("_sec1", np.array(C33), np.array(Q33))):
            dC, dQ = torch.from_numpy(com).cuda(), torch.from_numpy(pr).cuda()
            torch.cuda.synchronize()
            host = lambda ll, seed: getattr(L, "bppp_reciprocal_agg_verify_batch_rlc" + suffix)(
                ctx, label, ll, n, k, shape[1], shape[2], com.ctypes.data, pr.ctypes.data, *shape_of(case), acc.ctypes.data, st.ctypes.data, seed)
            device = lambda ll, seed: getattr(L, "bppp_reciprocal_agg_verify_batch_rlc" + suffix + "_device")(
                ctx, label, ll, n, k, shape[1], shape[2], dC.data_ptr(), dQ.data_ptr(), *shape_of(case), dA.data_ptr(), dS.data_ptr(), None, seed)
            for f in (host, device):
                assert f(len(label), None) == E, (shape, suffix)
                assert f(too_long, SEEDS[0]) == E, (shape, suffix)
                assert f(len(label), SEEDS[0]) == _capi.OK, (shape, suffix)
            v.synchronize()
            assert (acc == exp_acc).all() and (dA.cpu().numpy() == exp_acc).all(), (shape, suffix)
            # the exact wire forms and the wire provers look at the label too
            if suffix == "_sec1":
                assert L.bppp_reciprocal_agg_verify_batch_sec1(ctx, label, too_long, n, k, shape[1], shape[2], com.ctypes.data, pr.ctypes.data,
                                                               *shape_of(case), acc.ctypes.data, st.ctypes.data) == E
                assert L.bppp_reciprocal_agg_verify_batch_sec1_device(ctx, label, too_long, n, k, shape[1], shape[2], dC.data_ptr(), dQ.data_ptr(),
                                                                      *shape_of(case), dA.data_ptr(), dS.data_ptr(), None) == E
        buf = np.zeros(1 << 16, np.uint8)
        p = buf.ctypes.data
        assert L.bppp_reciprocal_agg_prove_values_batch_sec1(ctx, label, too_long, 1, k, shape[1], shape[2], p, p, p, p, p, p) == E
        assert L.bppp_reciprocal_agg_prove_values_batch_seeded_sec1(ctx, label, too_long, 1, k, shape[1], shape[2], p, p, SEEDS[0], 0, p, p, p) == E
        assert L.bppp_reciprocal_agg_prove_values_batch_seeded_sec1(ctx, label, len(label), 1, k, shape[1], shape[2], p, p, None, 0, p, p, p) == E
