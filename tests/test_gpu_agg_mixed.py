"""Aggregated reciprocal range proofs of mixed value counts in one batch on the GPU (bppp_reciprocal_agg_verify_batch_mixed[_device];
csrc/agg_mixed_core.h, k_agg_mixed.hip) against the oracle's verdict on every row (tests/golden/agg_mixed_cases.json, made by
tests/golden/make_agg_mixed_cases.py; the batch is described in tests/agg_mixed_cases.py).

Context shapes (k_max, nd, np) and the value counts of their instances, each the smallest to reach its edge:
    (3, 4, 4)     1, 2, 3      5, 6, 7 points of C0: one chunk of five, one more, two more; k_i = 1 on the aggregate's kernels;
                               k_i nd = 4, 8, 12 entries under 16 generators
    (7, 3, 4)     1 .. 7       5 to 11 points over one to three chunks; k_i nd = 3 .. 21 under 32: lane-group runs that end before the padding
    (6, 2, 3)     1 .. 6       np = nd + 1 (the entry cl_tau[nd] is not zero)
    (16, 16, 16)  1, 9, 15, 16 the real shape: 256 + 32 generators, 6 rounds; runs of 128 / 32 entries against k_i nd = 16, 144, 240
Every context is built with fb_window_bits = 8."""
import numpy as np
import pytest

import agg_cases as A
import agg_mixed_cases as M
from generic_forms import L1, L8, W
from test_agg_oracle import agg_expected_form

pytestmark = pytest.mark.gpu

SWEEP = (3, 4, 4)
# one size per launch form (the uniform call's sweep in tests/test_gpu_agg.py covers the plan at every threshold +- 1):
# phase 1 on 8 | 4 | 2 | 1 lanes, the fixed-base sums on a wavefront | 8 lanes | one lane, `beside` on | off, tables in 4 | 1 parts
SWEEP_CASES = [(1, -1), (8, 0), (8, 1), (16, 1), (32, 1), (128, 0)]


def _make(shape, **env):
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol
    case = A.setup(*shape)
    with pytest.MonkeyPatch.context() as mp:
        for key, v in env.items():
            mp.setenv(key, v)
        return AggregatedReciprocalRangeProofProtocol(shape[0], shape[1], shape[2], case["g"], case["gv"], case["hv"], case["gv_"],
                                                      case["hv_"], device=0, fb_window_bits=8)


@pytest.fixture(scope="module")
def verifiers():
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    made = {}
    try:
        for shape in M.CONTEXTS:
            made[shape] = _make(shape)
        yield made
    finally:
        for v in made.values():
            v.close()


def _device(v, case, ks, Cn, Qn, mixed=True):
    """-> (accept, status, reject count) of the device form; an instance no kernel reached keeps status 7."""
    import torch
    n = Cn.shape[0]
    own = lambda a, dt=np.uint8: np.require(a, dt, ["C", "W"])      # (the fixture's arrays are read-only)
    dC, dQ = torch.from_numpy(own(Cn)).cuda(), torch.from_numpy(own(Qn)).cuda()
    dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dS = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    dR = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    shape = (case["rounds"], case["nl"], case["nn"], dA.data_ptr(), dS.data_ptr(), dR.data_ptr())
    torch.cuda.synchronize()
    if mixed:
        dK = torch.from_numpy(own(ks)).cuda()
        torch.cuda.synchronize()
        v.verify_batch_mixed_device(case["label"], n, dK.data_ptr(), dC.data_ptr(), dQ.data_ptr(), *shape)
    else:
        v.verify_batch_device(case["label"], n, dC.data_ptr(), dQ.data_ptr(), *shape)
    v.synchronize()
    torch.cuda.synchronize()
    return dA.cpu().numpy(), dS.cpu().numpy(), int(dR.cpu()[0])


def _assert_rows(acc, st, exp_acc, exp_flag, tag):
    wrong = np.flatnonzero(acc != exp_acc)
    assert wrong.size == 0, (tag, "accept bits differ at", wrong[:16].tolist(), acc[wrong[:16]].tolist(), st[wrong[:16]].tolist())
    wrong = np.flatnonzero((st != 0) != exp_flag)
    assert wrong.size == 0, (tag, "statuses differ at", wrong[:16].tolist(), st[wrong[:16]].tolist())
    assert ((st & 1 != 0) == exp_flag).all(), tag       # the flagged rows are the malformed ones: BPPP_ST_BAD_ENCODING


@pytest.mark.parametrize("shape", list(M.CONTEXTS))
def test_every_row_vs_oracle_host_and_device(verifiers, shape):
    case, ks, Cn, Qn, exp_acc, exp_flag, notes = M.batch(shape)
    v = verifiers[shape]
    acc, st = v.verify_batch_mixed(case["label"], ks, Cn, Qn, case["rounds"], case["nl"], case["nn"])
    _assert_rows(acc, st, exp_acc, exp_flag, (shape, "host"))
    assert v._w.generic_form()["protocol"] == "aggregate"
    dacc, dst, rejects = _device(v, case, ks, Cn, Qn)
    assert dacc.tobytes() == acc.tobytes() and dst.tobytes() == st.tobytes(), shape
    assert rejects == int((exp_acc == 0).sum()) and 0 < rejects < M.ROWS
    noted = dict(notes)
    assert all(acc[r] == 1 for r in range(M.ROWS) if noted.get(r, "clean") in ("clean", "unused_ff", "unused_other"))


@pytest.mark.parametrize("shape,k", [((3, 4, 4), 2), ((16, 16, 16), 16)])
def test_all_equal_ks_gives_the_uniform_calls_bytes(shape, k):
    """The rows of one value count through the mixed call on the k_max context and through verify_batch[_device] with k on a context of
    the same generators: accept, status and reject count byte for byte, host and device forms."""
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol
    case_k, ks, Cn, Qn, exp_acc, exp_flag = M.uniform_batch(shape, k)
    assert len(ks) >= 8 and 0 < int((exp_acc == 0).sum()) < len(ks)
    Cd, Qd = np.ascontiguousarray(Cn[:, :k]), np.ascontiguousarray(Qn[:, :case_k["proof_bytes"]])
    shp = (case_k["rounds"], case_k["nl"], case_k["nn"])
    vm = _make(shape)
    vu = AggregatedReciprocalRangeProofProtocol(k, shape[1], shape[2], case_k["g"], case_k["gv"], case_k["hv"], case_k["gv_"], case_k["hv_"],
                                                device=0, fb_window_bits=8)
    try:
        uacc, ust = vu.verify_batch(case_k["label"], Cd, Qd, *shp)
        macc, mst = vm.verify_batch_mixed(case_k["label"], ks, Cn, Qn, *shp)
        _assert_rows(uacc, ust, exp_acc, exp_flag, (shape, k, "uniform"))
        assert macc.tobytes() == uacc.tobytes() and mst.tobytes() == ust.tobytes()
        ud, md = _device(vu, case_k, None, Cd, Qd, mixed=False), _device(vm, case_k, ks, Cn, Qn)
        assert md[0].tobytes() == ud[0].tobytes() == uacc.tobytes() and md[1].tobytes() == ud[1].tobytes() == ust.tobytes() and md[2] == ud[2]
    finally:
        vm.close()
        vu.close()


def test_k_max_1_gives_the_reciprocal_verifiers_bytes():
    """k_max = 1: the mixed call runs the aggregate's kernels on one value; the bytes are bppp_reciprocal_verify_batch's."""
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol, ReciprocalRangeProofProtocol
    shape = (3, 4, 4)
    case1, ks, Cn, Qn, exp_acc, exp_flag = M.uniform_batch(shape, 1)
    Cd, Qd = np.ascontiguousarray(Cn[:, :1]), np.ascontiguousarray(Qn[:, :case1["proof_bytes"]])
    shp = (case1["rounds"], case1["nl"], case1["nn"])
    gens = (case1["g"], case1["gv"], case1["hv"], case1["gv_"], case1["hv_"])
    r = ReciprocalRangeProofProtocol(4, 4, *gens, device=0, fb_window_bits=8)
    v = AggregatedReciprocalRangeProofProtocol(1, 4, 4, *gens, device=0, fb_window_bits=8)
    try:
        racc, rst = r.verify_batch(case1["label"], Cd.reshape(-1, 64), Qd, *shp)
        acc, st = v.verify_batch_mixed(case1["label"], ks, Cd, Qd, *shp)
        assert v._w.generic_form()["protocol"] == "aggregate"
        dacc, dst, rejects = _device(v, case1, ks, Cd, Qd)
        assert acc.tobytes() == racc.tobytes() == dacc.tobytes() and st.tobytes() == rst.tobytes() == dst.tobytes()
        assert rejects == int((racc == 0).sum())
        _assert_rows(acc, st, exp_acc, exp_flag, "k_max = 1")
    finally:
        r.close()
        v.close()


def test_device_counts_outside_the_range_flag_their_row_only(verifiers):
    shape = (7, 3, 4)
    case, ks, Cn, Qn, exp_acc, exp_flag, _ = M.batch(shape)
    v = verifiers[shape]
    ref = _device(v, case, ks, Cn, Qn)
    bad = ks.copy()
    rows = [1, 6, M.ROWS - 2]
    bad[1], bad[6], bad[M.ROWS - 2] = 0, shape[0] + 1, 255
    assert all(exp_acc[r] == 1 for r in rows[:2])
    acc, st, rejects = _device(v, case, bad, Cn, Qn)
    keep = np.setdiff1d(np.arange(M.ROWS), rows)
    assert (acc[rows] == 0).all() and (st[rows] & 1 == 1).all()
    assert acc[keep].tobytes() == ref[0][keep].tobytes() and st[keep].tobytes() == ref[1][keep].tobytes()
    assert rejects == int((acc == 0).sum())
    from bp_pp_amd import _capi
    with pytest.raises(_capi.BpppError) as e:            # the host form reads ks and refuses the call
        v.verify_batch_mixed(case["label"], bad, Cn, Qn, case["rounds"], case["nl"], case["nn"])
    assert e.value.code == _capi.ERR_INVALID_ARG


@pytest.mark.parametrize("group", ["2", "4"])
def test_phase1_lane_groups_on_the_sixteen_value_context(group):
    """BPPP_GENERIC_LANE_GROUP = 2 | 4: phase 1 on 2 | 8 lanes per instance at any size: runs of 128 | 32 entries against
    k_i nd = 16, 144, 240, 256, and the padding's pieces."""
    shape = (16, 16, 16)
    case, ks, Cn, Qn, exp_acc, exp_flag, _ = M.batch(shape)
    v = _make(shape, BPPP_GENERIC_LANE_GROUP=group)
    try:
        acc, st, _ = _device(v, case, ks, Cn, Qn)
        _assert_rows(acc, st, exp_acc, exp_flag, (shape, group))
        assert v._w.generic_form()["phase1_group"] == {"2": 2, "4": 8}[group]
    finally:
        v.close()


def test_projective_table_form_of_c0_on_mixed_counts():
    """BPPP_GENERIC_SLOW_ROUNDS: C0's variable-base sum over 4 + k_i points on projective tables; with kernel timing on (one stream) the
    stages are timed under the aggregate's names."""
    shape = (7, 3, 4)
    case, ks, Cn, Qn, exp_acc, exp_flag, _ = M.batch(shape)
    v = _make(shape, BPPP_GENERIC_SLOW_ROUNDS="1")
    try:
        acc, st = v.verify_batch_mixed(case["label"], ks, Cn, Qn, case["rounds"], case["nl"], case["nn"])
        _assert_rows(acc, st, exp_acc, exp_flag, (shape, "slow"))
        assert v._w.generic_form()["beside"] == 0
        v.enable_timing(True)
        v.timings()
        dacc, dst, _ = _device(v, case, ks, Cn, Qn)
        kt = v.timings()
        v.enable_timing(False)
        assert dacc.tobytes() == acc.tobytes() and dst.tobytes() == st.tobytes()
        for name in ("k_agg_phase1", "k_agg_c0_fixed", "k_agg_c0_var", "k_agg_c0_finish", "k_wnla_msm"):
            assert kt[name]["launches"] == 1, name
    finally:
        v.close()


def _repeated(shape, n):
    """The batch repeated to n rows; the last row is the batch's last corrupted one (what a short grid drops)."""
    case, ks, Cn, Qn, exp_acc, exp_flag, _ = M.batch(shape)
    idx = np.arange(n) % M.ROWS
    idx[n - 1] = M.ROWS - 1
    return case, ks[idx], np.ascontiguousarray(Cn[idx]), np.ascontiguousarray(Qn[idx]), exp_acc[idx], exp_flag[idx]


def test_parts_of_max_batch_take_their_own_slice_of_ks(verifiers):
    v = verifiers[(3, 4, 4)]
    case, ks, Cn, Qn, exp_acc, exp_flag = _repeated((3, 4, 4), 1024 + 70)
    assert (ks[1024:] != ks[:70]).any()                   # (a part that took the call's first counts would be wrong at once)
    before = v.get_option("max_batch")
    v.set_option("max_batch", 1024)
    try:
        acc, st, rejects = _device(v, case, ks, Cn, Qn)
        _assert_rows(acc, st, exp_acc, exp_flag, "device parts")
        assert rejects == int((exp_acc == 0).sum())
        acc, st = v.verify_batch_mixed(case["label"], ks, Cn, Qn, case["rounds"], case["nl"], case["nn"])
        _assert_rows(acc, st, exp_acc, exp_flag, "host parts")
    finally:
        v.set_option("max_batch", before)


_seen = {}


@pytest.mark.parametrize("T,d", SWEEP_CASES)
def test_launch_forms_vs_oracle(verifiers, T, d):
    v = verifiers[SWEEP]
    n = T * v.get_option("n_simds") + d
    case, ks, Cn, Qn, exp_acc, exp_flag = _repeated(SWEEP, n)
    acc, st, rejects = _device(v, case, ks, Cn, Qn)
    form = v._w.generic_form()
    _assert_rows(acc, st, exp_acc, exp_flag, (T, d))
    assert rejects == int((exp_acc == 0).sum()) and acc[n - 1] == 0
    assert form == agg_expected_form(T, d, case["rounds"]), (T, d, form)
    _seen[(T, d)] = form


def test_every_launch_form_was_entered(verifiers):
    for T, d in SWEEP_CASES:
        if (T, d) not in _seen:
            test_launch_forms_vs_oracle(verifiers, T, d)
    forms = lambda key: {f[key] for f in _seen.values()}
    assert forms("phase1_group") == {8, 4, 2, 1} and forms("fixed_base") == {W, L8, L1} and forms("beside") == {0, 1}
    assert forms("tab_parts") >= {4, 1} and forms("protocol") == {"aggregate"}


def test_argument_checks_on_a_live_context(verifiers):
    """The refusals of tests/test_agg_mixed_abi.py on a context: before anything touches the GPU (the buffers are never read)."""
    from bp_pp_amd import _capi
    L, E = _capi.lib(), _capi.ERR_INVALID_ARG
    v = verifiers[(16, 16, 16)]
    ctx = v._w._ctx
    buf = np.ones(1 << 16, np.uint8)
    p = buf.ctypes.data
    assert (v._w.ng, v._w.nh) == (256, 32)

    def host(k_max, nd, np_, ks=p, rounds=6, nl=1, nn=4, n=1):
        return L.bppp_reciprocal_agg_verify_batch_mixed(ctx, b"x", 1, n, k_max, ks, nd, np_, p, p, rounds, nl, nn, p, p)

    def dev(k_max, nd, np_, ks=p, rounds=6, nl=1, nn=4):
        return L.bppp_reciprocal_agg_verify_batch_mixed_device(ctx, b"x", 1, 0, k_max, ks, nd, np_, p, p, rounds, nl, nn, p, p, None)

    for f in (host, dev):
        assert f(16, 16, 16, ks=None) == E
        assert f(0, 16, 16) == E and f(65, 1, 1) == E and f(16, 17, 16) == E and f(64, 5, 4) == E and f(2, 23, 16) == E
        assert f(16, 16, 18) == E and f(16, 16, 16, rounds=13) == E and f(16, 16, 16, nl=4097) == E and f(16, 16, 16, nn=4097) == E
    zero, big = np.zeros(4, np.uint8), np.full(4, 17, np.uint8)
    assert host(16, 16, 16, ks=zero.ctypes.data) == E and host(16, 16, 16, ks=big.ctypes.data) == E
    assert host(64, 4, 5, n=0) == 0 and dev(64, 4, 5) == 0 and dev(11, 22, 23) == 0 and dev(16, 16, 17, rounds=12, nl=4096, nn=4096) == 0
    assert L.bppp_reciprocal_agg_verify_batch_mixed_device(ctx, b"x", 1, 1, 16, p, 16, 16, p, p, 6, 1, 4, p, None, None) == E      # d_status
