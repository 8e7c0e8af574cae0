"""The aggregated reciprocal range proof in the wire (SEC1) form on the GPU: bppp_reciprocal_agg_verify_batch_sec1[_device] and
bppp_reciprocal_agg_prove_values_batch[_seeded]_sec1.

Verifier: the wire batch is wire.pack of the golden batch (agg_golden.batch: 70 rows, one corrupted row per field class, the oracle's
verdict on every row).  Three of those rows are damaged by an off-curve 64-byte point, which has no compressed form; they carry an
undecodable encoding in the same field instead, cycling through the kinds of test_gpu_generic_sec1.bad_encodings (bad tag, x = p,
x = 2^256 - 1, x^3 + 7 a non-residue), and the oracle (agg_cases.verify) is asked about the expanded row.  The host and the device
form must give the 64-byte twin's accept bits, statuses and reject count on wire.expand of the same bytes, and the oracle's verdicts.

"max_batch" takes no value below 1024, so the call in two parts behind one expansion is 1024 + 6 rows with "max_batch" = 1024 (a
second part shorter than a chunk of 8, as 70 rows in parts of 64 would leave), and the prover's n = 5 runs as two parts at
(16, 16, 16) only, where 1024 multiplication gates are 4 instances.

Prover: the wire outputs are wire.pack of the 64-byte provers' outputs on the same inputs (tests/agg_prove_cases.py), proofs and
commitments, and verify_batch_sec1 accepts them."""
import functools

import numpy as np
import pytest

import agg_cases as A
import agg_golden
import agg_prove_cases as AP
from bp_pp_amd import wire
from test_gpu_generic_sec1 import bad_encodings

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 4), (2, 4, 4), (6, 2, 3), (16, 16, 16)]
OFF_CURVE_KINDS = ("R_off_curve", "V_off_curve", "coordinate_p")
UNDECODABLE = (0, 2, 3, 4)                     # bad_encodings: tag 04, x = p, x = 2^256 - 1, a non-residue x (5 is the identity)
ST_BAD_ENCODING, ST_OUT_OF_RANGE = 1, 4
SEED = bytes.fromhex("243f6a8885a308d313198a2e03707344a4093822299f31d0082efa98ec4e6c89")
PARTS_ROWS = 1024 + 6


def n_points(case):
    return 4 + 2 * case["rounds"] + case["k"]


def shape_of(case):
    return case["rounds"], case["nl"], case["nn"]


def undecodable(valid33: bytes, i: int) -> np.ndarray:
    return np.frombuffer(bad_encodings(bytes(valid33))[UNDECODABLE[i % len(UNDECODABLE)]][0], np.uint8)


def expand(case, C33, Q33):
    """The 64-byte form the device expands a wire batch to."""
    k = case["k"]
    n = C33.shape[0]
    return (wire.expand(C33.reshape(n, -1), k).reshape(n, k, 64), wire.expand(Q33, n_points(case), case["nl"] + case["nn"]))


@functools.lru_cache(maxsize=None)
def wire_batch(shape):
    """(case, C33 [70, k, 33], Q33 [70, wire bytes], expect_acc, expect_flag): the golden batch packed, the three off-curve rows with
    undecodable encodings in their place and the oracle's verdict on those rows' expansion.  Made once; never written to."""
    case, Cn, Qn, exp_acc, exp_flag, kinds = agg_golden.batch(shape)
    k, rounds, P, S = case["k"], case["rounds"], n_points(case), case["nl"] + case["nn"]
    C33 = wire.pack(Cn.reshape(A.ROWS, -1), k).reshape(A.ROWS, k, 33)
    Q33 = wire.pack(Qn, P, S)
    exp_acc, exp_flag = exp_acc.copy(), exp_flag.copy()
    field = {"R_off_curve": 4 + 2 * rounds + k // 2, "coordinate_p": 2}          # the point of the proof each kind damages
    differ = []
    for i, kind in enumerate(OFF_CURVE_KINDS):
        row = dict((name, r) for r, name in kinds)[kind]
        if kind == "V_off_curve":
            C33[row, k - 1] = undecodable(C33[0, k - 1], i)
        else:
            j = field[kind]
            Q33[row, 33 * j:33 * j + 33] = undecodable(Q33[0, 33 * j:33 * j + 33], i)
        differ.append(row)
    C64, Q64 = expand(case, C33, Q33)
    same = np.setdiff1d(np.arange(A.ROWS), differ)
    assert C64[same].tobytes() == Cn[same].tobytes() and Q64[same].tobytes() == Qn[same].tobytes()
    for row in differ:
        rc = A.verify(case, C64[row].tobytes(), Q64[row].tobytes())
        assert rc == -1, (shape, row, rc)          # k256 would not have deserialised it
        exp_acc[row], exp_flag[row] = 0, True
    for a in (C33, Q33, exp_acc, exp_flag):
        a.setflags(write=False)
    return case, C33, Q33, exp_acc, exp_flag


def make(shape):
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol
    case = agg_golden.load(shape)[0]
    return AggregatedReciprocalRangeProofProtocol(shape[0], shape[1], shape[2], case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"],
                                                  device=0, fb_window_bits=8)


@pytest.fixture(scope="module")
def protos():
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    made = {}
    try:
        for shape in SHAPES:
            made[shape] = make(shape)
        yield made
    finally:
        for v in made.values():
            v.close()


def device_call(v, case, Cn, Qn, method="verify_batch_sec1_device", seed=None):
    """A device form over torch tensors -> (accept, status, reject count); an instance no kernel reached keeps status 7."""
    import torch
    n = Cn.shape[0]
    dC, dQ = torch.from_numpy(np.array(Cn, copy=True)).cuda(), torch.from_numpy(np.array(Qn, copy=True)).cuda()
    dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dS = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    dR = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    tail = () if seed is None else (seed,)
    getattr(v, method)(case["label"], n, dC.data_ptr(), dQ.data_ptr(), *shape_of(case), dA.data_ptr(), dS.data_ptr(), *tail, dR.data_ptr())
    v.synchronize()
    torch.cuda.synchronize()
    return dA.cpu().numpy(), dS.cpu().numpy(), int(dR.cpu()[0])


def assert_rows(acc, st, exp_acc, exp_flag, tag):
    wrong = np.flatnonzero(acc != exp_acc)
    assert wrong.size == 0, (tag, "accept bits differ at", wrong[:16].tolist())
    wrong = np.flatnonzero((st != 0) != exp_flag)
    assert wrong.size == 0, (tag, "statuses differ at", wrong[:16].tolist(), st[wrong[:16]].tolist())
    assert ((st & ST_BAD_ENCODING != 0) == exp_flag).all(), (tag, st[exp_flag].tolist())          # the flagged rows are the malformed ones


def check_wire_call(v, case, C33, Q33, exp_acc, exp_flag, tag):
    """Host and device SEC1 forms against the 64-byte twins on the expanded bytes and against the expected verdicts."""
    C64, Q64 = expand(case, C33, Q33)
    acc64, st64 = v.verify_batch(case["label"], C64, Q64, *shape_of(case))
    _, _, rej64 = device_call(v, case, C64, Q64, "verify_batch_device")
    acc, st = v.verify_batch_sec1(case["label"], C33, Q33, *shape_of(case))
    dacc, dst, rej = device_call(v, case, C33, Q33)
    assert acc.tobytes() == acc64.tobytes() and st.tobytes() == st64.tobytes(), (tag, "host vs the 64-byte twin")
    assert dacc.tobytes() == acc64.tobytes() and dst.tobytes() == st64.tobytes(), (tag, "device vs the 64-byte twin")
    assert rej == rej64 == int((exp_acc == 0).sum()), (tag, rej, rej64)
    assert_rows(acc, st, exp_acc, exp_flag, tag)
    return acc, st


@pytest.mark.parametrize("shape", SHAPES)
def test_wire_batch_equals_the_64_byte_twin_and_the_oracle(protos, shape):
    case, C33, Q33, exp_acc, exp_flag = wire_batch(shape)
    v = protos[shape]
    assert Q33.shape[1] == v.proof_sec1_bytes(*shape_of(case)) == 33 * n_points(case) + 32 * (case["nl"] + case["nn"])
    check_wire_call(v, case, C33, Q33, exp_acc, exp_flag, shape)
    assert int(exp_flag.sum()) == len(OFF_CURVE_KINDS)
    if shape[0] > 1:
        assert v._w.generic_form()["protocol"] == "aggregate"


def _valid_rows(shape, n):
    """n rows of the wire batch's accepted rows, repeated."""
    case, C33, Q33, exp_acc, _ = wire_batch(shape)
    idx = np.flatnonzero(exp_acc == 1)[np.arange(n) % int(exp_acc.sum())]
    return case, C33[idx].copy(), Q33[idx].copy()


def test_an_undecodable_point_in_every_position_class_and_the_identity(protos):
    shape = (2, 4, 4)
    v = protos[shape]
    case, C33, Q33 = _valid_rows(shape, 48)
    k, r = case["k"], case["rounds"]
    R0 = 4 + 2 * r
    # c_l c_r c_o c_s, the first and last r, the first and last x, the first, middle and last R; then the first and last V
    proof_positions = [0, 1, 2, 3, 4, 4 + r - 1, 4 + r, R0 - 1, R0, R0 + k // 2, R0 + k - 1]
    flagged = []
    row = 1
    for i, j in enumerate(proof_positions):
        Q33[row, 33 * j:33 * j + 33] = undecodable(Q33[row, 33 * j:33 * j + 33], i)
        flagged.append(row); row += 3
    for i, j in enumerate((0, k - 1)):
        C33[row, j] = undecodable(C33[row, j], len(proof_positions) + i)
        flagged.append(row); row += 3
    identity_row = row
    Q33[identity_row, 33 * R0:33 * R0 + 33] = 0                  # the identity at R_0: 64 zero bytes to the twin
    assert identity_row + 1 < 48
    C64, Q64 = expand(case, C33, Q33)
    assert not Q64[identity_row, 64 * R0:64 * R0 + 64].any()
    exp_acc, exp_flag = np.ones(48, np.uint8), np.zeros(48, bool)
    exp_acc[flagged], exp_flag[flagged] = 0, True
    rc = A.verify(case, C64[identity_row].tobytes(), Q64[identity_row].tobytes())
    exp_acc[identity_row], exp_flag[identity_row] = (1 if rc == 1 else 0), rc < 0
    acc, st = check_wire_call(v, case, C33, Q33, exp_acc, exp_flag, "positions")
    neighbours = np.setdiff1d(np.arange(48), flagged + [identity_row])
    assert acc[neighbours].all() and not st[neighbours].any()


def test_the_ragged_tail_of_the_flat_lane_map(protos):
    shape = (2, 4, 4)
    case, C33, Q33, exp_acc, exp_flag = wire_batch(shape)
    idx = np.arange(257) % A.ROWS
    check_wire_call(protos[shape], case, C33[idx], Q33[idx], exp_acc[idx], exp_flag[idx], "257 rows")


def test_two_parts_behind_one_expansion(protos):
    shape = (2, 4, 4)
    v = protos[shape]
    case, C33, Q33, exp_acc, exp_flag = wire_batch(shape)
    idx = np.arange(PARTS_ROWS) % A.ROWS
    idx[-1] = A.ROWS - 1                                          # the call's last row: a corrupted one, in the short second part
    before = v.get_option("max_batch")
    v.set_option("max_batch", 1024)
    try:
        check_wire_call(v, case, C33[idx], Q33[idx], exp_acc[idx], exp_flag[idx], "two parts")
    finally:
        v.set_option("max_batch", before)


def test_k1_equals_the_reciprocal_wire_verifier_on_the_same_bytes(protos):
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    shape = (1, 4, 4)
    case, C33, Q33, exp_acc, exp_flag = wire_batch(shape)
    r = ReciprocalRangeProofProtocol(4, 4, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0, fb_window_bits=8)
    try:
        racc, rst = r.verify_batch_sec1(case["label"], C33.reshape(-1, 33), Q33, *shape_of(case))
    finally:
        r.close()
    v = protos[shape]
    acc, st = v.verify_batch_sec1(case["label"], C33, Q33, *shape_of(case))
    dacc, dst, rejects = device_call(v, case, C33, Q33)
    assert acc.tobytes() == racc.tobytes() == dacc.tobytes() and st.tobytes() == rst.tobytes() == dst.tobytes()
    assert rejects == int((racc == 0).sum())
    assert v._w.generic_form()["protocol"] == "reciprocal"
    assert_rows(acc, st, exp_acc, exp_flag, shape)


def _pack_outputs(case, proofs, com):
    k = case["k"]
    n = proofs.shape[0]
    return wire.pack(proofs, n_points(case), case["nl"] + case["nn"]), wire.pack(com.reshape(n, -1), k).reshape(n, k, 33)


@pytest.mark.parametrize("shape", [(1, 4, 4), (2, 4, 4), (16, 16, 16)])
def test_prover_wire_output_is_the_64_byte_output_compressed(protos, shape):
    """(1, 4, 4): the k = 1 forward, the reciprocal prover from integers with its outputs compressed."""
    k, nd, np_ = shape
    p = protos[shape]
    case, _, pool, _ = agg_golden.load(shape)
    n = 5
    x, s, rnd = AP.batch(case, [b % len(pool) for b in range(n)], p.prove_draws())
    assert p.proof_shape() == shape_of(case)
    x = x.copy()
    x[3, k // 2] = np.frombuffer(AP.be32(np_**nd), np.uint8)               # one above the range: instance 3 alone is flagged
    calls = [("rnd", lambda: p.prove_values_batch(case["label"], x, s, rnd), lambda: p.prove_values_batch_sec1(case["label"], x, s, rnd)),
             ("seeded", lambda: p.prove_values_batch_seeded(case["label"], x, s, SEED, 11),
              lambda: p.prove_values_batch_seeded_sec1(case["label"], x, s, SEED, 11))]
    for tag, twin, sec1 in calls:
        want, wcom, wst, _ = twin()
        got, gcom, st, pshape = sec1()
        assert pshape == shape_of(case) and st.tobytes() == wst.tobytes(), (shape, tag)
        assert st.tolist() == [0, 0, 0, ST_OUT_OF_RANGE, 0], (shape, tag, st.tolist())
        want33, wcom33 = _pack_outputs(case, want, wcom)
        assert got.tobytes() == want33.tobytes() and gcom.tobytes() == wcom33.tobytes(), (shape, tag)
        assert not got[3].any() and not gcom[3].any() and got[[0, 1, 2, 4]].any(axis=1).all() and gcom[[0, 1, 2, 4]].any(axis=(1, 2)).all()
        acc, vst = p.verify_batch_sec1(case["label"], gcom, got, *pshape)
        assert acc.tolist() == [1, 1, 1, 0, 1] and not vst[[0, 1, 2, 4]].any(), (shape, tag, acc.tolist(), vst.tolist())
    if k * nd == 256:
        # 1024 multiplication gates a part: 4 instances, so n = 5 runs as two parts; the seeded streams go on from part to part
        want, wcom, wst, _ = calls[1][1]()
        before = p.get_option("max_batch")
        p.set_option("max_batch", 1024)
        try:
            got, gcom, st, _ = calls[1][2]()
            got_r, gcom_r, st_r, _ = calls[0][2]()
        finally:
            p.set_option("max_batch", before)
        want33, wcom33 = _pack_outputs(case, want, wcom)
        assert got.tobytes() == want33.tobytes() and gcom.tobytes() == wcom33.tobytes() and st.tobytes() == wst.tobytes()
        want_r, wcom_r, _, _ = calls[0][1]()
        want33, wcom33 = _pack_outputs(case, want_r, wcom_r)
        assert got_r.tobytes() == want33.tobytes() and gcom_r.tobytes() == wcom33.tobytes() and st_r.tobytes() == wst.tobytes()


def test_an_empty_call_zeroes_the_reject_count_at_every_route(protos):
    """n = 0 through the wire device forms: the counter reads 0 at k > 1, at the k = 1 forward and at k = 1 over the u64 generators
    (the route to the u64 kernels)."""
    import torch
    import workload
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol
    g, gv, hv = workload.split_generators(workload.make_batch(1, first=0)[0])
    u64 = AggregatedReciprocalRangeProofProtocol(1, 16, 16, g, gv, hv[:26], [], hv[26:], device=0, fb_window_bits=8)
    try:
        buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        dS = torch.zeros(1, dtype=torch.int32, device="cuda")
        for v, shape3 in ((protos[(2, 4, 4)], (3, 2, 1)), (protos[(1, 4, 4)], (2, 2, 1)), (u64, (4, 2, 1))):
            for method, tail in (("verify_batch_sec1_device", ()), ("verify_batch_rlc_sec1_device", (SEED,))):
                dR = torch.full((1,), -1, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                getattr(v, method)(b"x", 0, buf.data_ptr(), buf.data_ptr(), *shape3, buf.data_ptr(), dS.data_ptr(), *tail, dR.data_ptr())
                v.synchronize()
                torch.cuda.synchronize()
                assert int(dR.cpu()[0]) == 0, (v.k, v.dim_nd, method)
    finally:
        u64.close()
