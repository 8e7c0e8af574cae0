"""The aggregated reciprocal range proof verifier on the GPU (bppp_reciprocal_agg_verify_batch[_device]; csrc/agg_core.h, k_agg.hip)
against the oracle's verdicts on every row (tests/golden/agg_cases.json, made by tests/golden/make_agg_cases.py).

Shapes (k, nd, np), each the smallest to hit its edge:
    (1, 4, 4)     must equal bppp_reciprocal_verify_batch on the same bytes: accept, status and reject count
    (2, 4, 4)     6 points of C0: one full chunk of five and one more
    (3, 4, 4)     nm = 12 padded to 16; 7 points
    (6, 2, 3)     10 points: two full chunks; np = nd + 1 (the entry cl_tau[nd] is not zero)
    (7, 3, 4)     11 points: three chunks; nm = 21 padded to 32
    (16, 16, 16)  sixteen u64 values: 256 + 32 generators, 6 rounds
Batches are agg_cases.ROWS = 70 rows with one row corrupted per field class (agg_cases.corrupted_batch).  The launch forms -- phase 1
on 8, 4, 2, 1 lanes, the fixed-base sums on a wavefront, 8 lanes and one lane, `beside` on and off -- are entered at their own
thresholds - 1, + 0, + 1 with the (2, 4, 4) batch repeated, as tests/test_gpu_generic_boundaries.py does for the older verifiers."""
import ctypes as C

import numpy as np
import pytest

import agg_cases as A
import agg_golden
from generic_forms import L1, L8, RECIP_ONLY, THRESHOLDS, W
from test_agg_oracle import agg_expected_form

pytestmark = pytest.mark.gpu

SWEEP = (2, 4, 4)
CASES = [(T, d) for T in THRESHOLDS + [RECIP_ONLY] for d in (-1, 0, 1)]
_seen = {}


def _make(shape, **env):
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol
    case = agg_golden.load(shape)[0]
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return AggregatedReciprocalRangeProofProtocol(shape[0], shape[1], shape[2], case["g"], case["gv"], case["hv"], case["gv_"],
                                                      case["hv_"], device=0, fb_window_bits=8)


@pytest.fixture(scope="module")
def verifiers():
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    made = {}
    try:
        for shape in A.SHAPES:
            made[shape] = _make(shape)
        yield made
    finally:
        for v in made.values():
            v.close()


def _device_verify(v, case, Cn, Qn):
    import torch
    n = Cn.shape[0]
    dC, dQ = torch.from_numpy(Cn).cuda(), torch.from_numpy(Qn).cuda()
    dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dS = torch.full((n,), 7, dtype=torch.int32, device="cuda")          # (an instance no kernel reached keeps the 7)
    dR = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    v.verify_batch_device(case["label"], n, dC.data_ptr(), dQ.data_ptr(), case["rounds"], case["nl"], case["nn"], dA.data_ptr(), dS.data_ptr(),
                          dR.data_ptr())
    v.synchronize()
    torch.cuda.synchronize()
    return dA.cpu().numpy(), dS.cpu().numpy(), int(dR.cpu()[0])


def _assert_rows(acc, st, exp_acc, exp_flag, tag):
    wrong = np.flatnonzero(acc != exp_acc)
    assert wrong.size == 0, (tag, "accept bits differ at", wrong[:16].tolist())
    wrong = np.flatnonzero((st != 0) != exp_flag)
    assert wrong.size == 0, (tag, "statuses differ at", wrong[:16].tolist(), st[wrong[:16]].tolist())
    assert ((st & 1 != 0) == exp_flag).all(), tag       # the flagged rows are the malformed ones: BPPP_ST_BAD_ENCODING


@pytest.mark.parametrize("shape", A.SHAPES)
def test_every_corrupted_field_class_vs_oracle_host_and_device(verifiers, shape):
    case, Cn, Qn, exp_acc, exp_flag, kinds = agg_golden.batch(shape)
    v = verifiers[shape]
    acc, st = v.verify_batch(case["label"], Cn, Qn, case["rounds"], case["nl"], case["nn"])
    _assert_rows(acc, st, exp_acc, exp_flag, (shape, "host"))
    dacc, dst, rejects = _device_verify(v, case, Cn, Qn)
    assert dacc.tobytes() == acc.tobytes() and dst.tobytes() == st.tobytes(), shape
    assert rejects == int((exp_acc == 0).sum()) == len(kinds)
    if shape[0] > 1:
        assert v._w.generic_form()["protocol"] == "aggregate"


def test_k1_equals_the_reciprocal_verifier_on_the_same_bytes(verifiers):
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    shape = (1, 4, 4)
    case, Cn, Qn, exp_acc, exp_flag, _ = agg_golden.batch(shape)
    r = ReciprocalRangeProofProtocol(4, 4, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0, fb_window_bits=8)
    try:
        racc, rst = r.verify_batch(case["label"], Cn.reshape(-1, 64), Qn, case["rounds"], case["nl"], case["nn"])
    finally:
        r.close()
    acc, st = verifiers[shape].verify_batch(case["label"], Cn, Qn, case["rounds"], case["nl"], case["nn"])
    dacc, dst, rejects = _device_verify(verifiers[shape], case, Cn, Qn)
    assert acc.tobytes() == racc.tobytes() == dacc.tobytes() and st.tobytes() == rst.tobytes() == dst.tobytes()
    assert rejects == int((racc == 0).sum())
    assert verifiers[shape]._w.generic_form()["protocol"] == "reciprocal"
    _assert_rows(acc, st, exp_acc, exp_flag, shape)


def _sweep_batch(n):
    """The (2, 4, 4) batch of 70 repeated to n rows; the last row is the batch's last corrupted one (what a short grid drops)."""
    case, Cn, Qn, exp_acc, exp_flag, _ = agg_golden.batch(SWEEP)
    idx = np.arange(n) % A.ROWS
    idx[n - 1] = A.ROWS - 1
    return case, np.ascontiguousarray(Cn[idx]), np.ascontiguousarray(Qn[idx]), exp_acc[idx], exp_flag[idx]


def _run_case(verifiers, T, d):
    v = verifiers[SWEEP]
    n = T * v.get_option("n_simds") + d
    case, Cn, Qn, exp_acc, exp_flag = _sweep_batch(n)
    acc, st, rejects = _device_verify(v, case, Cn, Qn)
    form = v._w.generic_form()
    _assert_rows(acc, st, exp_acc, exp_flag, (T, d))
    assert rejects == int((exp_acc == 0).sum()) and acc[n - 1] == 0
    assert form == agg_expected_form(T, d, case["rounds"]), (T, d, form)
    _seen[(T, d)] = tuple(sorted(form.items()))


@pytest.mark.parametrize("T,d", CASES)
def test_launch_forms_at_their_thresholds_vs_oracle(verifiers, T, d):
    _run_case(verifiers, T, d)


def test_every_launch_form_was_entered(verifiers):
    for T, d in CASES:
        if (T, d) not in _seen:
            _run_case(verifiers, T, d)
    forms = lambda key: {dict(f)[key] for f in _seen.values()}
    assert forms("phase1_group") == {8, 4, 2, 1} and forms("fixed_base") == {W, L8, L1} and forms("beside") == {0, 1}
    assert forms("tab_parts") == {4, 2, 1} and forms("round_group") == {16, 8, 4, 2, 1} and forms("protocol") == {"aggregate"}


@pytest.mark.parametrize("shape", [(7, 3, 4), (16, 16, 16)])
def test_projective_table_form_of_c0_and_kernel_timing(shape):
    """BPPP_GENERIC_SLOW_ROUNDS: C0's variable-base sum (and the rounds) on projective tables with complete additions -- the form the
    plan takes when it is not `fast`; and with kernel timing on (one stream, no `beside`) the new kernels are named in the timing table."""
    case, Cn, Qn, exp_acc, exp_flag, _ = agg_golden.batch(shape)
    v = _make(shape, BPPP_GENERIC_SLOW_ROUNDS="1")
    try:
        acc, st = v.verify_batch(case["label"], Cn, Qn, case["rounds"], case["nl"], case["nn"])
        _assert_rows(acc, st, exp_acc, exp_flag, (shape, "slow"))
        assert v._w.generic_form()["beside"] == 0
        v.enable_timing(True)
        v.timings()
        dacc, dst, _ = _device_verify(v, case, Cn, Qn)
        kt = v.timings()
        v.enable_timing(False)
        assert dacc.tobytes() == acc.tobytes() and dst.tobytes() == st.tobytes()
        for name in ("k_agg_phase1", "k_agg_c0_fixed", "k_agg_c0_var", "k_agg_c0_finish", "k_wnla_msm"):
            assert kt[name]["launches"] == 1, name
        assert kt["k_wnla_round"]["launches"] == case["rounds"] and kt["k_recip_phase1"]["launches"] == 0
    finally:
        v.close()


@pytest.mark.parametrize("group", ["2", "4"])
def test_phase1_lane_groups_on_the_sixteen_value_shape(group):
    """BPPP_GENERIC_LANE_GROUP = 2 | 4: phase 1 on 2 | 8 lanes per instance at any size, on the shape whose runs of 128 | 32 entries
    cross value boundaries of 16."""
    shape = (16, 16, 16)
    case, Cn, Qn, exp_acc, exp_flag, _ = agg_golden.batch(shape)
    v = _make(shape, BPPP_GENERIC_LANE_GROUP=group)
    try:
        acc, st, _ = _device_verify(v, case, Cn, Qn)
        _assert_rows(acc, st, exp_acc, exp_flag, (shape, group))
        assert v._w.generic_form()["phase1_group"] == {"2": 2, "4": 8}[group]
    finally:
        v.close()


def test_parts_of_max_batch_and_allocation_failure(verifiers):
    """A call of more than "max_batch" instances runs as consecutive parts; an allocation that fails is BPPP_ERR_NOMEM and the next
    call is served."""
    from bp_pp_amd import _capi
    v = verifiers[(3, 4, 4)]
    case, Cn, Qn, exp_acc, exp_flag, _ = agg_golden.batch((3, 4, 4))
    n = 1024 + 70
    idx = np.arange(n) % A.ROWS
    Cn, Qn, exp_acc, exp_flag = np.ascontiguousarray(Cn[idx]), np.ascontiguousarray(Qn[idx]), exp_acc[idx], exp_flag[idx]
    before = v.get_option("max_batch")
    v.set_option("max_batch", 1024)
    try:
        acc, st, rejects = _device_verify(v, case, Cn, Qn)
        _assert_rows(acc, st, exp_acc, exp_flag, "device parts")
        assert rejects == int((exp_acc == 0).sum())
        acc, st = v.verify_batch(case["label"], Cn, Qn, case["rounds"], case["nl"], case["nn"])
        _assert_rows(acc, st, exp_acc, exp_flag, "host parts")
    finally:
        v.set_option("max_batch", before)
    big = np.ascontiguousarray(np.tile(Cn, (3, 1, 1))), np.ascontiguousarray(np.tile(Qn, (3, 1)))      # (larger than any call so far: the blob grows)
    v.set_option("inject_alloc_fault", 1)
    with pytest.raises(_capi.BpppError) as e:
        v.verify_batch(case["label"], big[0], big[1], case["rounds"], case["nl"], case["nn"])
    assert e.value.code == _capi.ERR_NOMEM
    acc, st = v.verify_batch(case["label"], Cn, Qn, case["rounds"], case["nl"], case["nn"])
    _assert_rows(acc, st, exp_acc, exp_flag, "after NOMEM")


def test_argument_checks_at_their_edges(verifiers):
    """Every bound at its edge is BPPP_ERR_INVALID_ARG, before anything touches the GPU (the buffers are never read)."""
    from bp_pp_amd import _capi
    L = _capi.lib()
    E = _capi.ERR_INVALID_ARG
    v = verifiers[(16, 16, 16)]                      # 256 generators in g_vec, 32 in h_vec
    ctx = v._w._ctx
    buf = np.zeros(1 << 16, np.uint8)
    p = buf.ctypes.data
    assert (v._w.ng, v._w.nh) == (256, 32)

    def host(k, nd, np_, rounds=6, nl=1, nn=4, n=1):
        return L.bppp_reciprocal_agg_verify_batch(ctx, b"x", 1, n, k, nd, np_, p, p, rounds, nl, nn, p, p)

    def dev(k, nd, np_, rounds=6, nl=1, nn=4):
        return L.bppp_reciprocal_agg_verify_batch_device(ctx, b"x", 1, 0, k, nd, np_, p, p, rounds, nl, nn, p, p, None)

    for f in (host, dev):
        assert f(0, 16, 16) == E and f(65, 1, 1) == E                 # 1 <= k <= 64
        assert f(16, 17, 16) == E and f(64, 5, 4) == E                # k dim_nd <= |g_vec| (16 x 17 = 272, 64 x 5 = 320 > 256)
        assert f(2, 23, 16) == E                                      # dim_nd + 10 <= |h_vec| (33 > 32)
        assert f(16, 16, 18) == E and f(16, 0, 1) == E and f(16, 16, 0) == E      # dim_np <= dim_nd + 1, nothing empty
        assert f(16, 16, 16, rounds=13) == E and f(16, 16, 16, nl=4097) == E and f(16, 16, 16, nn=4097) == E
    # ... and the edges themselves pass the checks (n = 0: nothing to do)
    assert host(64, 4, 5, n=0) == 0 and dev(64, 4, 5) == 0 and dev(11, 22, 23) == 0 and dev(16, 16, 17, rounds=12, nl=4096, nn=4096) == 0
    assert L.bppp_reciprocal_agg_verify_batch(None, b"x", 1, 1, 2, 4, 4, p, p, 3, 2, 1, p, p) == E
    assert L.bppp_reciprocal_agg_verify_batch(ctx, b"x", 1, 1, 2, 4, 4, None, p, 3, 2, 1, p, p) == E
    assert L.bppp_reciprocal_agg_verify_batch_device(ctx, b"x", 1, 1, 2, 4, 4, p, p, 3, 2, 1, p, None, None) == E      # d_status is required
    assert L.bppp_reciprocal_agg_proof_bytes(16, 6, 1, 4) == 2208 and L.bppp_reciprocal_agg_proof_bytes(1, 4, 2, 1) == 928
    assert C.sizeof(C.c_size_t) == 8
