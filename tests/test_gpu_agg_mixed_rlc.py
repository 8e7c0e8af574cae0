"""The RLC mode of the mixed-value-count aggregate verifier on the GPU (bppp_reciprocal_agg_verify_batch_mixed_rlc[_sec1][_device]),
after tests/test_gpu_agg_rlc.py: accept bits, statuses and reject count equal the exact mixed call's on every row, on prefixes of the
batch of tests/agg_mixed_cases.py around the chunk of 8 -- 1 and 7 (no complete chunk: the exact final sum, reported as (0, 0)), 8, 9
and all 71 rows with their ragged tail -- with the bucket stage over superchunks of 64, in parts of "max_batch", and over the wire form.

"max_batch" takes no value below 1024, so the call in parts is 1024 + 6 rows with "max_batch" = 1024: the second part has fewer
than 8 instances and runs the exact sum, while the call reports the first part's chunk of 8."""
import numpy as np
import pytest

import agg_mixed_cases as M
import agg_mixed_wire_cases as MW
from agg_mixed_wire_cases import shape_of
from test_gpu_agg_mixed_sec1 import PARTS_ROWS, assert_rows, device_call, make

pytestmark = pytest.mark.gpu

SHAPES = [(3, 4, 4), (6, 2, 3), (16, 16, 16)]
SIZES = (1, 7, 8, 9, M.ROWS)
CHUNK = 8
SUPER = 64                                   # the smallest superchunk "rlc_superchunk" takes
N_SUPER = 2 * SUPER + 3
SEEDS = (bytes(range(7, 39)), bytes(range(200, 232)))
RLC_KERNELS = ("k_wnla_rlc_lhs", "k_wnla_rlc_chunk", "k_wnla_rlc_check", "k_bkt_prepare", "k_bkt_accumulate", "k_bkt_scalars", "k_bkt_check")


@pytest.fixture(scope="module")
def verifiers():
    """Per shape one context that chooses its superchunk by itself; "fixed": one whose "rlc_superchunk" the tests set (the option cannot
    be put back to automatic)."""
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    made = {}
    try:
        for shape in SHAPES:
            made[shape] = make(shape)
        made["fixed"] = make((3, 4, 4))
        yield made
    finally:
        for v in made.values():
            v.close()


def _used(v):
    return v.get_option("last_rlc_superchunk"), v.get_option("last_rlc_chunk")


def _check(v, case, ks, Cn, Qn, exp_acc, exp_flag, used, tag):
    """Both seeds through the host and the device RLC form, the exact mixed call before them: byte-equal, and the expected verdicts."""
    args = (case["label"], ks, Cn, Qn, *shape_of(case))
    acc_e, st_e = v.verify_batch_mixed(*args)
    assert_rows(acc_e, st_e, exp_acc, exp_flag, (tag, "exact vs expected"))
    rej_e = int((acc_e == 0).sum())
    for seed in SEEDS:
        acc, st = v.verify_batch_mixed_rlc(*args, seed)
        assert _used(v) == used, (tag, _used(v))
        assert acc.tobytes() == acc_e.tobytes() and st.tobytes() == st_e.tobytes(), (tag, "rlc host", acc.tolist(), st.tolist())
        dacc, dst, rej = device_call(v, case, ks, Cn, Qn, "verify_batch_mixed_rlc_device", seed)
        assert _used(v) == used, (tag, _used(v))
        assert dacc.tobytes() == acc_e.tobytes() and dst.tobytes() == st_e.tobytes(), (tag, "rlc device", dacc.tolist(), dst.tolist())
        assert rej == rej_e, (tag, rej, rej_e)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", SHAPES)
def test_rlc_equals_exact_on_prefixes_around_the_chunk_size(verifiers, shape, n):
    """The automatic superchunk is 256 at these sizes: one ragged superchunk in front of the chunks of 8.  last_rlc_chunk is what tells
    the chunk stage from a call that ran the exact sums."""
    case, ks, Cn, Qn, exp_acc, exp_flag, _ = M.batch(shape)
    used = (256, CHUNK) if n >= CHUNK else (0, 0)
    _check(verifiers[shape], case, ks[:n], np.ascontiguousarray(Cn[:n]), np.ascontiguousarray(Qn[:n]), exp_acc[:n], exp_flag[:n], used,
           (shape, n))


@pytest.mark.parametrize("shape,k", [((3, 4, 4), 2), ((16, 16, 16), 16)])
def test_all_equal_ks_gives_the_uniform_rlc_calls_bytes_and_chunks(shape, k):
    case_k, ks, Cn, Qn, exp_acc, exp_flag = M.uniform_batch(shape, k)
    assert len(ks) >= CHUNK
    Cd, Qd = np.ascontiguousarray(Cn[:, :k]), np.ascontiguousarray(Qn[:, :case_k["proof_bytes"]])
    vm, vu = make(shape), make((k, shape[1], shape[2]), case_k)
    try:
        uacc, ust = vu.verify_batch_rlc(case_k["label"], Cd, Qd, *shape_of(case_k), SEEDS[0])
        u_used = _used(vu)
        macc, mst = vm.verify_batch_mixed_rlc(case_k["label"], ks, Cn, Qn, *shape_of(case_k), SEEDS[0])
        assert _used(vm) == u_used and u_used[1] == CHUNK
        assert_rows(uacc, ust, exp_acc, exp_flag, (shape, k, "uniform"))
        assert macc.tobytes() == uacc.tobytes() and mst.tobytes() == ust.tobytes()
        ud = device_call(vu, case_k, None, Cd, Qd, "verify_batch_rlc_device", SEEDS[0])
        md = device_call(vm, case_k, ks, Cn, Qn, "verify_batch_mixed_rlc_device", SEEDS[0])
        assert _used(vm) == _used(vu) == u_used
        assert md[0].tobytes() == ud[0].tobytes() == uacc.tobytes() and md[1].tobytes() == ud[1].tobytes() == ust.tobytes() and md[2] == ud[2]
    finally:
        vm.close()
        vu.close()


def _valid_tiled(shape, n):
    """n clean rows, ks cycling through the shape's counts."""
    case, ks, Cn, Qn, exp_acc, _, _ = M.batch(shape)
    idx = np.arange(n) % M.CLEAN
    assert exp_acc[:M.CLEAN].all() and len(set(ks[idx[:8]].tolist())) == len(M.CONTEXTS[shape])
    return case, ks[idx].copy(), np.ascontiguousarray(Cn[idx]), np.ascontiguousarray(Qn[idx])


def _scalar_end(case, k):
    return case["proof_bytes"] if k == case["k"] else M.setup_on(case, k)["proof_bytes"]


def _tamper(case, ks, Q, i):
    """Well-formed and wrong: a bit flipped in the row's last proof scalar (never its top byte: the value stays below the group order)."""
    Q[i, _scalar_end(case, int(ks[i])) - 32 + 17] ^= 0x10


def _malform(Q, i):
    """A bad encoding: the first round point off the curve."""
    Q[i, 256 + 63] ^= 1


def test_rlc_bucket_stage_on_two_superchunks_and_a_ragged_one(verifiers):
    shape = (3, 4, 4)
    v = verifiers["fixed"]
    n = N_SUPER
    case, ks, Cn, Q0 = _valid_tiled(shape, n)
    batches = [("all valid", Q0, [], [])]
    Q = Q0.copy()
    _tamper(case, ks, Q, 11)
    _tamper(case, ks, Q, SUPER + 9)
    _tamper(case, ks, Q, n - 1)                   # one tampered scalar at a row of each superchunk
    batches.append(("one tampered scalar in each superchunk", Q, [11, SUPER + 9, n - 1], []))
    Q = Q.copy()
    _malform(Q, 20)                               # then one malformed point: a flagged instance has weight zero
    batches.append(("and one malformed point", Q, [11, SUPER + 9, n - 1], [20]))
    v.set_option("rlc_superchunk", SUPER)
    for what, Q, bad, flagged in batches:
        exp_acc, exp_flag = np.ones(n, np.uint8), np.zeros(n, bool)
        exp_acc[bad + flagged], exp_flag[flagged] = 0, True
        _check(v, case, ks, Cn, Q, exp_acc, exp_flag, (SUPER, CHUNK), what)


def test_rlc_kernels_show_in_the_timings(verifiers):
    """What shows that the chunk stage ran, rather than everything falling through to the exact sums."""
    shape = (3, 4, 4)
    v = verifiers[shape]
    case, ks, Cn, Qn, exp_acc, exp_flag, _ = M.batch(shape)
    v.enable_timing(True)
    try:
        v.timings()                                  # (reset)
        acc, st, _ = device_call(v, case, ks, Cn, Qn, "verify_batch_mixed_rlc_device", SEEDS[0])
        kt = v.timings()
        acc_e, st_e, _ = device_call(v, case, ks, Cn, Qn, "verify_batch_mixed_device")
        ke = v.timings()
    finally:
        v.enable_timing(False)
    assert_rows(acc, st, exp_acc, exp_flag, "timed")
    assert acc.tobytes() == acc_e.tobytes() and st.tobytes() == st_e.tobytes()
    for name in RLC_KERNELS:
        assert kt[name]["launches"] == 1, (name, kt.get(name))
        assert name not in ke or ke[name]["launches"] == 0, (name, ke.get(name))
    assert kt["k_wnla_msm"]["launches"] == 2 and kt["k_agg_phase1"]["launches"] == 1
    assert ke["k_wnla_msm"]["launches"] == 1 and ke["k_agg_phase1"]["launches"] == 1


def test_rlc_in_parts_of_max_batch(verifiers):
    shape = (3, 4, 4)
    v = verifiers[shape]
    case, ks, Cn, Qn, exp_acc, exp_flag, _ = M.batch(shape)
    idx = np.arange(PARTS_ROWS) % M.ROWS
    idx[-1] = M.ROWS - 1                              # the call's last row: a corrupted one, in the part that runs the exact sum
    before = v.get_option("max_batch")
    v.set_option("max_batch", 1024)
    try:
        _check(v, case, ks[idx], np.ascontiguousarray(Cn[idx]), np.ascontiguousarray(Qn[idx]), exp_acc[idx], exp_flag[idx], (256, CHUNK), "parts")
    finally:
        v.set_option("max_batch", before)


def test_rlc_over_the_wire_equals_the_exact_wire_call_and_rlc_on_the_expansion(verifiers):
    shape = (3, 4, 4)
    v = verifiers[shape]
    case, ks, C33, Q33, C64, Q64, exp_acc, exp_flag, _, _ = MW.wire_batch(shape)
    acc_e, st_e = v.verify_batch_mixed_sec1(case["label"], ks, C33, Q33, *shape_of(case))
    assert_rows(acc_e, st_e, exp_acc, exp_flag, "exact wire")
    for seed in SEEDS:
        acc, st = v.verify_batch_mixed_rlc_sec1(case["label"], ks, C33, Q33, *shape_of(case), seed)
        assert _used(v) == (256, CHUNK)
        dacc, dst, rej = device_call(v, case, ks, C33, Q33, "verify_batch_mixed_rlc_sec1_device", seed)
        assert _used(v) == (256, CHUNK)
        xacc, xst = v.verify_batch_mixed_rlc(case["label"], ks, C64, Q64, *shape_of(case), seed)
        assert acc.tobytes() == acc_e.tobytes() == dacc.tobytes() == xacc.tobytes()
        assert st.tobytes() == st_e.tobytes() == dst.tobytes() == xst.tobytes()
        assert rej == int((exp_acc == 0).sum())


def test_a_null_seed_is_refused_on_a_live_context(verifiers):
    """The C symbols themselves (the Python mirror refuses a seed of None before the call): with a context, buffers and sizes that pass
    every other check, a NULL seed alone is BPPP_ERR_INVALID_ARG; the same call with a seed is served."""
    import torch
    from bp_pp_amd import _capi
    L, E = _capi.lib(), _capi.ERR_INVALID_ARG
    shape = (3, 4, 4)
    v = verifiers[shape]
    ctx = v._w._ctx
    case, ks, C33, Q33, C64, Q64, exp_acc, _, _, _ = MW.wire_batch(shape)
    n, label = M.ROWS, case["label"]
    own = lambda a: np.array(a, np.uint8, copy=True)
    acc, st = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    dA, dS = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    kk = own(ks)
    dK = torch.from_numpy(kk).cuda()
    for suffix, com, pr in (("", own(C64), own(Q64)), ("_sec1", own(C33), own(Q33))):
        dC, dQ = torch.from_numpy(com).cuda(), torch.from_numpy(pr).cuda()
        torch.cuda.synchronize()
        host = lambda seed: getattr(L, "bppp_reciprocal_agg_verify_batch_mixed_rlc" + suffix)(
            ctx, label, len(label), n, shape[0], kk.ctypes.data, shape[1], shape[2], com.ctypes.data, pr.ctypes.data, *shape_of(case),
            acc.ctypes.data, st.ctypes.data, seed)
        device = lambda seed: getattr(L, "bppp_reciprocal_agg_verify_batch_mixed_rlc" + suffix + "_device")(
            ctx, label, len(label), n, shape[0], dK.data_ptr(), shape[1], shape[2], dC.data_ptr(), dQ.data_ptr(), *shape_of(case),
            dA.data_ptr(), dS.data_ptr(), None, seed)
        for f in (host, device):
            assert f(None) == E, suffix
            assert f(SEEDS[0]) == _capi.OK, suffix
        v.synchronize()
        assert (acc == exp_acc).all() and (dA.cpu().numpy() == exp_acc).all(), suffix


def _one_or_two_values(wire):
    """The rows of the (3, 4, 4) batch with one or two values, in slots laid out by k_max = 2 on that context's generators (an
    instance is verified by its own count whatever the slots): (case, ks, commitments, proofs, accept, flagged) by the oracle."""
    if wire:
        case_max, ks, C, Q, _, _, exp_acc, exp_flag, _, _ = MW.wire_batch((3, 4, 4))
    else:
        case_max, ks, C, Q, exp_acc, exp_flag, _ = M.batch((3, 4, 4))
    case = M.setup_on(case_max, 2)
    idx = np.flatnonzero(ks <= 2)
    assert set(ks[idx].tolist()) == {1, 2} and 0 < int(exp_acc[idx].sum()) < len(idx) and exp_flag[idx].any()
    width = MW.sec1_bytes(case_max, 2) if wire else case["proof_bytes"]
    return case, ks[idx].copy(), np.ascontiguousarray(C[idx, :2]), np.ascontiguousarray(Q[idx, :width]), exp_acc[idx], exp_flag[idx]


@pytest.mark.parametrize("form", ["host", "device", "sec1", "rlc"])
def test_allocation_failure_at_every_position_is_nomem_and_the_context_recovers(form):
    """After tests/test_gpu_agg_rlc.py, for the mixed family: a call larger than any before it -- 64 rows more each time, so that the
    projective tables, the bucket buffers and the workspace or staging all grow -- with the first, then the second, then the third ...
    device allocation failing, for as long as the call still fails.  Each failure is ERR_NOMEM, leaves no stale "last_rlc_*", and the
    next call is served with the oracle's rows.  How many positions a form has is printed, not pinned."""
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    from bp_pp_amd._capi import ERR_NOMEM, BpppError
    case, ks, Cn, Qn, exp_acc, exp_flag = _one_or_two_values(form == "sec1")
    args = shape_of(case)
    call = {"host": lambda v, k, c, q: v.verify_batch_mixed(case["label"], k, c, q, *args),
            "device": lambda v, k, c, q: device_call(v, case, k, c, q, "verify_batch_mixed_device")[:2],
            "sec1": lambda v, k, c, q: v.verify_batch_mixed_sec1(case["label"], k, c, q, *args),
            "rlc": lambda v, k, c, q: v.verify_batch_mixed_rlc(case["label"], k, c, q, *args, SEEDS[0])}[form]
    rlc = form == "rlc"
    v = make((2, 4, 4), case)
    try:
        acc, st = call(v, ks, Cn, Qn)
        assert_rows(acc, st, exp_acc, exp_flag, (form, "before"))
        assert not rlc or _used(v) == (256, CHUNK)
        positions = 0
        for fault in range(1, 9):
            big = np.arange(64 * (fault + 1) + 7) % len(ks)
            v.set_option("inject_alloc_fault", fault)
            try:
                acc, st = call(v, ks[big], Cn[big], Qn[big])
            except BpppError as e:
                assert e.code == ERR_NOMEM, (form, fault, e.code)
                acc = None
            v.set_option("inject_alloc_fault", 0)
            if acc is not None:                           # fewer allocations than `fault`: the call was served
                assert_rows(acc, st, exp_acc[big], exp_flag[big], (form, fault, "served"))
                break
            positions += 1
            assert not rlc or _used(v) == (0, 0), (form, fault)      # nothing stale after the failure
            acc, st = call(v, ks, Cn, Qn)                 # the next call is served
            assert_rows(acc, st, exp_acc, exp_flag, (form, fault, "after"))
            assert not rlc or _used(v) == (256, CHUNK), (form, fault)
        else:
            pytest.fail("%s: a call still fails with the 9th allocation as the failing one" % form)
        print("allocation-fault positions of the mixed %s form: %d" % (form, positions))
        assert positions >= 1, form                       # the call grew something
    finally:
        v.close()
