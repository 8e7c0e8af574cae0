"""Aggregated reciprocal range proofs of mixed value counts in the wire (SEC1) form on the GPU
(bppp_reciprocal_agg_verify_batch_mixed_sec1[_device]; csrc/wire_mixed_core.h, k_wire_mixed.hip) on the wire batch of
tests/agg_mixed_wire_cases.py: the host and the device form give the 64-byte mixed call's accept bits, statuses and reject count on
the Python expansion of the same bytes, and the oracle's verdict on every row.

Context shapes (k_max, nd, np) and the value counts of their instances, as in tests/test_gpu_agg_mixed.py:
    (3, 4, 4)     1, 2, 3      5, 6, 7 points of C0: one chunk of five, one more, two more
    (7, 3, 4)     1 .. 7       5 to 11 points over one to three chunks; lane-group runs that end before the padding
    (6, 2, 3)     1 .. 6       np = nd + 1
    (16, 16, 16)  1, 9, 15, 16 the real shape: 256 + 32 generators, 6 rounds
Every context is built with fb_window_bits = 8.  "max_batch" takes no value below 1024, so the call in two parts behind one expansion
is 1024 + 6 rows with "max_batch" = 1024."""
import numpy as np
import pytest

import agg_cases as A
import agg_mixed_cases as M
import agg_mixed_wire_cases as MW
from agg_mixed_wire_cases import shape_of

pytestmark = pytest.mark.gpu

PARTS_ROWS = 1024 + 6


def make(shape, case=None):
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol
    case = case or A.setup(*shape)
    return AggregatedReciprocalRangeProofProtocol(shape[0], shape[1], shape[2], case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"],
                                                  device=0, fb_window_bits=8)


@pytest.fixture(scope="module")
def verifiers():
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    made = {}
    try:
        for shape in M.CONTEXTS:
            made[shape] = make(shape)
        yield made
    finally:
        for v in made.values():
            v.close()


def device_call(v, case, ks, Cn, Qn, method="verify_batch_mixed_sec1_device", seed=None):
    """A device form over torch tensors (ks None: a uniform call) -> (accept, status, reject count); an instance no kernel reached
    keeps status 7."""
    import torch
    n = Cn.shape[0]
    up = lambda a: torch.from_numpy(np.array(a, np.uint8, copy=True)).cuda()
    dC, dQ = up(Cn), up(Qn)
    dK = () if ks is None else (up(ks),)
    dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dS = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    dR = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tail = () if seed is None else (seed,)
    getattr(v, method)(case["label"], n, *(t.data_ptr() for t in dK), dC.data_ptr(), dQ.data_ptr(), *shape_of(case), dA.data_ptr(),
                       dS.data_ptr(), *tail, dR.data_ptr())
    v.synchronize()
    torch.cuda.synchronize()
    return dA.cpu().numpy(), dS.cpu().numpy(), int(dR.cpu()[0])


def assert_rows(acc, st, exp_acc, exp_flag, tag):
    wrong = np.flatnonzero(acc != exp_acc)
    assert wrong.size == 0, (tag, "accept bits differ at", wrong[:16].tolist(), acc[wrong[:16]].tolist(), st[wrong[:16]].tolist())
    wrong = np.flatnonzero((st != 0) != exp_flag)
    assert wrong.size == 0, (tag, "statuses differ at", wrong[:16].tolist(), st[wrong[:16]].tolist())
    assert ((st & 1 != 0) == exp_flag).all(), tag       # the flagged rows are the malformed ones: BPPP_ST_BAD_ENCODING


def check_wire_call(v, case, ks, C33, Q33, C64, Q64, exp_acc, exp_flag, tag):
    """Host and device SEC1 forms against the 64-byte mixed twins on the expansion and against the expected verdicts."""
    acc64, st64 = v.verify_batch_mixed(case["label"], ks, C64, Q64, *shape_of(case))
    _, _, rej64 = device_call(v, case, ks, C64, Q64, "verify_batch_mixed_device")
    acc, st = v.verify_batch_mixed_sec1(case["label"], ks, C33, Q33, *shape_of(case))
    dacc, dst, rej = device_call(v, case, ks, C33, Q33)
    assert acc.tobytes() == acc64.tobytes() and st.tobytes() == st64.tobytes(), (tag, "host vs the 64-byte twin")
    assert dacc.tobytes() == acc64.tobytes() and dst.tobytes() == st64.tobytes(), (tag, "device vs the 64-byte twin")
    assert rej == rej64 == int((exp_acc == 0).sum()), (tag, rej, rej64)
    assert_rows(acc, st, exp_acc, exp_flag, tag)
    return acc, st


@pytest.mark.parametrize("shape", list(M.CONTEXTS))
def test_wire_batch_equals_the_64_byte_twin_and_the_oracle(verifiers, shape):
    case, ks, C33, Q33, C64, Q64, exp_acc, exp_flag, notes, asked = MW.wire_batch(shape)
    v = verifiers[shape]
    assert Q33.shape[1] == v.proof_sec1_bytes(*shape_of(case)) == MW.sec1_bytes(case, shape[0])
    acc, st = check_wire_call(v, case, ks, C33, Q33, C64, Q64, exp_acc, exp_flag, shape)
    assert v._w.generic_form()["protocol"] == "aggregate"
    what = dict(notes)
    assert all(acc[r] == 1 for r in range(M.ROWS) if what.get(r, "clean") in ("clean", "unused_ff", "unused_other"))
    assert 0 < int((exp_acc == 0).sum()) < M.ROWS and int(exp_flag.sum()) >= 6


def _uniform_rows(shape, k):
    """The rows of the wire batch whose ks is k, cut to the uniform wire layout for k: (case_k, ks, C33 slots, Q33 slots, C33 [m, k, 33],
    Q33 [m, S(k)])"""
    case_max, ks, C33, Q33 = MW.wire_batch(shape)[:4]
    idx = np.flatnonzero(ks == k)
    case_k = M.setup_on(case_max, k)
    Cs, Qs = np.ascontiguousarray(C33[idx]), np.ascontiguousarray(Q33[idx])
    return case_k, ks[idx].copy(), Cs, Qs, np.ascontiguousarray(Cs[:, :k]), np.ascontiguousarray(Qs[:, :MW.sec1_bytes(case_max, k)])


@pytest.mark.parametrize("shape,k", [((3, 4, 4), 2), ((16, 16, 16), 16)])
def test_all_equal_ks_gives_the_uniform_wire_calls_bytes(shape, k):
    """The rows of one value count through the mixed wire call on the k_max context and through verify_batch_sec1[_device] with k on a
    context of the same generators: accept, status and reject count byte for byte."""
    case_k, ks, Cs, Qs, Cd, Qd = _uniform_rows(shape, k)
    assert len(ks) >= 8
    vm, vu = make(shape), make((k, shape[1], shape[2]), case_k)
    try:
        uacc, ust = vu.verify_batch_sec1(case_k["label"], Cd, Qd, *shape_of(case_k))
        macc, mst = vm.verify_batch_mixed_sec1(case_k["label"], ks, Cs, Qs, *shape_of(case_k))
        assert 0 < int((uacc == 0).sum()) < len(ks)
        assert macc.tobytes() == uacc.tobytes() and mst.tobytes() == ust.tobytes()
        ud = device_call(vu, case_k, None, Cd, Qd, "verify_batch_sec1_device")
        md = device_call(vm, case_k, ks, Cs, Qs)
        assert md[0].tobytes() == ud[0].tobytes() == uacc.tobytes() and md[1].tobytes() == ud[1].tobytes() == ust.tobytes() and md[2] == ud[2]
    finally:
        vm.close()
        vu.close()


def test_k_max_1_gives_the_reciprocal_wire_verifiers_bytes():
    """k_max = 1: nothing is forwarded, the mixed kernels run on one value; the bytes are bppp_reciprocal_verify_batch_sec1's."""
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    shape = (3, 4, 4)
    case1, ks, _, _, Cd, Qd = _uniform_rows(shape, 1)
    gens = (case1["g"], case1["gv"], case1["hv"], case1["gv_"], case1["hv_"])
    r = ReciprocalRangeProofProtocol(4, 4, *gens, device=0, fb_window_bits=8)
    v = make((1, 4, 4), case1)
    try:
        racc, rst = r.verify_batch_sec1(case1["label"], Cd.reshape(-1, 33), Qd, *shape_of(case1))
        acc, st = v.verify_batch_mixed_sec1(case1["label"], ks, Cd, Qd, *shape_of(case1))
        assert v._w.generic_form()["protocol"] == "aggregate"
        dacc, dst, rejects = device_call(v, case1, ks, Cd, Qd)
        assert acc.tobytes() == racc.tobytes() == dacc.tobytes() and st.tobytes() == rst.tobytes() == dst.tobytes()
        assert rejects == int((racc == 0).sum()) and 0 < rejects < len(ks)
    finally:
        r.close()
        v.close()


def test_device_counts_outside_the_range_flag_their_row_only(verifiers):
    shape = (7, 3, 4)
    case, ks, C33, Q33, _, _, exp_acc, _, _, _ = MW.wire_batch(shape)
    v = verifiers[shape]
    ref = device_call(v, case, ks, C33, Q33)
    bad = ks.copy()
    rows = [1, 6, M.ROWS - 2]
    bad[1], bad[6], bad[M.ROWS - 2] = 0, shape[0] + 1, 255
    assert all(exp_acc[r] == 1 for r in rows[:2])
    acc, st, rejects = device_call(v, case, bad, C33, Q33)
    keep = np.setdiff1d(np.arange(M.ROWS), rows)
    assert (acc[rows] == 0).all() and (st[rows] & 1 == 1).all()
    assert acc[keep].tobytes() == ref[0][keep].tobytes() and st[keep].tobytes() == ref[1][keep].tobytes()
    assert rejects == int((acc == 0).sum())
    C64, Q64 = MW.expand(case, bad, C33, Q33)              # and the 64-byte device form on the expansion of the same counts
    twin = device_call(v, case, bad, C64, Q64, "verify_batch_mixed_device")
    assert twin[0].tobytes() == acc.tobytes() and twin[1].tobytes() == st.tobytes() and twin[2] == rejects
    from bp_pp_amd import _capi
    with pytest.raises(_capi.BpppError) as e:             # the host form reads ks and refuses the call
        v.verify_batch_mixed_sec1(case["label"], bad, C33, Q33, *shape_of(case))
    assert e.value.code == _capi.ERR_INVALID_ARG


def test_two_parts_behind_one_expansion(verifiers):
    shape = (3, 4, 4)
    v = verifiers[shape]
    case, ks, C33, Q33, C64, Q64, exp_acc, exp_flag, _, _ = MW.wire_batch(shape)
    idx = np.arange(PARTS_ROWS) % M.ROWS
    idx[-1] = M.ROWS - 1                                   # the call's last row: a corrupted one, in the short second part
    assert (ks[idx][1024:] != ks[idx][:6]).any()          # (a part that took the call's first counts would be wrong at once)
    before = v.get_option("max_batch")
    v.set_option("max_batch", 1024)
    try:
        check_wire_call(v, case, ks[idx], C33[idx], Q33[idx], C64[idx], Q64[idx], exp_acc[idx], exp_flag[idx], "two parts")
    finally:
        v.set_option("max_batch", before)


def test_argument_checks_on_a_live_context(verifiers):
    """The mixed call's refusals, before anything touches the GPU (the buffers are never read); an empty call zeroes the counter."""
    import torch
    from bp_pp_amd import _capi
    L, E = _capi.lib(), _capi.ERR_INVALID_ARG
    v = verifiers[(16, 16, 16)]
    ctx = v._w._ctx
    buf = np.ones(1 << 16, np.uint8)
    p = buf.ctypes.data
    assert (v._w.ng, v._w.nh) == (256, 32)

    def host(k_max, nd, np_, ks=p, rounds=6, nl=1, nn=4, n=1, com=p, pr=p, acc=p):
        return L.bppp_reciprocal_agg_verify_batch_mixed_sec1(ctx, b"x", 1, n, k_max, ks, nd, np_, com, pr, rounds, nl, nn, acc, p)

    def dev(k_max, nd, np_, ks=p, rounds=6, nl=1, nn=4, n=0, com=p, pr=p, acc=p, st=p):
        return L.bppp_reciprocal_agg_verify_batch_mixed_sec1_device(ctx, b"x", 1, n, k_max, ks, nd, np_, com, pr, rounds, nl, nn, acc, st, None)

    for f in (host, dev):
        assert f(16, 16, 16, ks=None) == E and f(16, 16, 16, com=None) == E and f(16, 16, 16, pr=None) == E and f(16, 16, 16, acc=None) == E
        assert f(0, 16, 16) == E and f(65, 1, 1) == E and f(16, 17, 16) == E and f(64, 5, 4) == E and f(2, 23, 16) == E
        assert f(16, 16, 18) == E and f(16, 16, 16, rounds=13) == E and f(16, 16, 16, nl=4097) == E and f(16, 16, 16, nn=4097) == E
    assert dev(16, 16, 16, n=1, st=None) == E
    zero, big = np.zeros(4, np.uint8), np.full(4, 17, np.uint8)
    assert host(16, 16, 16, ks=zero.ctypes.data) == E and host(16, 16, 16, ks=big.ctypes.data) == E
    assert host(64, 4, 5, n=0) == 0 and dev(64, 4, 5) == 0 and dev(11, 22, 23) == 0
    dR = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    d = torch.zeros(64, dtype=torch.uint8, device="cuda").data_ptr()
    torch.cuda.synchronize()
    assert L.bppp_reciprocal_agg_verify_batch_mixed_sec1_device(ctx, b"x", 1, 0, 16, d, 16, 16, d, d, 6, 1, 4, d, d, dR.data_ptr()) == 0
    v.synchronize()
    assert int(dR.cpu()[0]) == 0
