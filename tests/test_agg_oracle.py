"""CPU tier for the aggregated reciprocal range proof: the protocol pinned on the oracle (tests/agg_cases.py builds the circuit on
bppp_oracle.ArithmeticCircuit), the golden file re-derived, and the verifier's launch plan (csrc/plan_core.h: plan_generic with
GENERIC_FORM_AGGREGATE) at its thresholds -- with the plans of the three older protocols shown unchanged."""
import numpy as np
import pytest

import agg_cases as A
import agg_golden
import bppp_oracle as O
from generic_forms import FORMS, RECIP_ONLY, THRESHOLDS

N = O.N


def test_k1_is_the_reciprocal_protocol_byte_for_byte():
    """Same generators, witness and prover scalars: the proof bytes and the verifier's trace of ReciprocalRangeProofProtocol."""
    case = A.setup(1, 4, 4)
    com, proof = A.prove(case, 5)
    digits = A.seeded_digits(case, 5)[0]
    x = sum(d * 4**i for i, d in enumerate(digits))
    s = A._sc(b"s", 5, 0)
    proto = O.ReciprocalRangeProofProtocol(dim_nd=4, dim_np=4, g=case["Pg"], g_vec=list(case["Pgv"]), h_vec=list(case["Phv"]),
                                           g_vec_=list(case["Pgv_"]), h_vec_=list(case["Phv_"]))
    cnt = [0]

    def rng():
        cnt[0] += 1
        return A._sc(b"rnd", 5, cnt[0])

    V = proto.commit_value(x, s)
    p = proto.prove(V, O.ReciprocalWitness(x=x, s=s, m=[digits.count(v) for v in range(4)], digits=digits), O.Transcript(case["label"]), rng)
    cp = p.circuit_proof
    blob = b"".join(O.pt_to_xy64(q) for q in [cp.c_l, cp.c_r, cp.c_o, cp.c_s] + list(cp.r) + list(cp.x) + [p.r])
    blob += b"".join(O.sc_to_bytes(v) for v in list(cp.l) + list(cp.n))
    assert O.pt_to_xy64(V) == com and blob == proof
    t1, t2 = [], []
    assert proto.verify(V, p, O.Transcript(case["label"]), t1) and A.verify(case, com, proof, t2) == 1
    d1, d2 = dict(t1), dict(t2)
    assert d2["V+R"] == [d1["V+r"]]
    for key in ("e", "rho", "lambda", "beta", "delta", "tau", "pn_tau", "ps_tau", "c", "C0"):
        assert d1[key] == d2[key], key
    assert [v for k, v in t1 if k.startswith("wnla")] == [v for k, v in t2 if k.startswith("wnla")]


@pytest.mark.parametrize("shape", [(1, 4, 4), (2, 4, 4), (3, 4, 4), (5, 3, 4), (6, 2, 3), (7, 3, 4)])
def test_valid_instances_accept(shape):
    case = A.setup(*shape)
    for b in (0, 1, 2):       # all digits 0, all np - 1, seeded
        com, proof = A.prove(case, b)
        assert len(com) == 64 * shape[0] and len(proof) == A.proof_bytes(shape[0], case["rounds"], case["nl"], case["nn"])
        assert A.verify(case, com, proof) == 1, (shape, b)


def test_proof_size_of_sixteen_u64_values():
    case = A.setup(16, 16, 16)
    assert (case["NG"], case["NH"], case["rounds"], case["nl"], case["nn"]) == (256, 32, 6, 1, 4)
    assert case["proof_bytes"] == 64 * (4 + 12 + 16) + 32 * 5 == 2208 and 16 * 928 == 14848


def test_dishonest_witnesses_and_mixed_up_inputs_reject():
    case = A.setup(3, 4, 4)
    k, nd, np_ = 3, 4, 4
    digits = A.seeded_digits(case, 7)
    honest = [sum(dg * np_**d for d, dg in enumerate(row)) for row in digits]
    # a value outside its range: the committed x_1 is np^nd more than its digits spell
    xs = list(honest)
    xs[1] += np_**nd
    assert A.verify(case, *A.prove(case, 7, xs=xs)) == 0
    # a digit >= np with honest reciprocals: the value and the reciprocals are of digit np, the multiplicities cannot count it
    bad = [list(r) for r in digits]
    bad[2][1] = np_
    assert A.verify(case, *A.prove(case, 7, digits=bad)) == 0
    com, proof = A.prove(case, 7)
    com2, proof2 = A.prove(case, 8)
    assert A.verify(case, com, proof) == 1 and A.verify(case, com2, proof2) == 1
    # V_0 and V_1 swapped
    assert A.verify(case, com[64:128] + com[:64] + com[128:], proof) == 0
    # an R_i taken from another instance
    o = A.field_offsets(case)["R_mid"]
    assert A.verify(case, com, proof[:o] + proof2[o:o + 64] + proof[o + 64:]) == 0


def test_dim_np_beyond_dim_nd_plus_one_is_not_a_valid_shape():
    """The existing rule dim_np <= dim_nd + 1: (3, 2, 4) proofs do not verify."""
    case = A.setup(3, 2, 4)
    assert A.verify(case, *A.prove(case, 2)) == 0


@pytest.mark.parametrize("shape", [s for s in A.SHAPES if s != (16, 16, 16)])
def test_the_golden_file_is_what_the_oracle_says(shape):
    """Instances accept; a sample of the corrupted rows' verdicts recomputed (the whole file: tests/golden/make_agg_cases.py)."""
    case, coms, proofs, corrupted = agg_golden.load(shape)
    assert A.prove(case, 3) == (coms[3].tobytes(), proofs[3].tobytes())
    assert A.verify(case, coms[4].tobytes(), proofs[4].tobytes()) == 1
    _, C, Q, acc, flag, kinds = agg_golden.batch(shape)
    sample = [(r, kind) for r, kind in kinds if kind in ("R_mid", "V_swapped", "R_off_curve", "V_eq_R", "V_eq_negR", "n_last_row")]
    for row, (a, f) in A.expectations(case, C, Q, sample).items():
        assert (a, f) == (int(acc[row]), bool(flag[row])), (shape, row)
    assert len(kinds) >= 19 and int(flag.sum()) == 3 and int((acc == 0).sum()) == len(kinds)


# ---- the launch plan
PROTOCOL = {"wnla": 1, "recip": 2, "circuit": 3}
SHAPE = {"wnla": (4, 0), "recip": (5, 0), "circuit": (2, 6)}          # rounds and C0 points of tests/test_generic_plan.py's sweep
AGGREGATE = 4
GRID_T = THRESHOLDS + [RECIP_ONLY]
# "last_generic_form" of the three older protocols over that sweep -- every threshold T (x 1,024 SIMDs) at T - 1, T, T + 1 instances,
# kernel timing off and on -- as plan_generic returned them BEFORE the aggregate form was added (recorded from the parent commit)
CODES_BEFORE = {
    1: [0x81e11, 0x81e11, 0x81e11, 0x81e11, 0x81d09, 0x81d09, 0x81d09, 0x81d09, 0x81d09, 0x81d09, 0x81c85, 0x81c85, 0x81c85, 0x81c85, 0x81c85, 0x81c85, 0x80c85, 0x80c85, 0x80c85, 0x80c85, 0x80c85, 0x80c85, 0x80c45, 0x80c45, 0x80c45, 0x80c45, 0x80c45, 0x80c45, 0x80825, 0x80825, 0x80825, 0x80825, 0x80825, 0x80825, 0x80425, 0x80425, 0x80425, 0x80425, 0x80425, 0x80425, 0x80025, 0x80025, ],
    2: [0xe1e12, 0xa1e12, 0xe1e12, 0xa1e12, 0xe1d0a, 0xa1d0a, 0xe1d0a, 0xa1d0a, 0xe1d0a, 0xa1d0a, 0xe1c86, 0xa1c86, 0xe1c86, 0xa1c86, 0xe1c86, 0xa1c86, 0xd0c86, 0x90c86, 0xd0c86, 0x90c86, 0xd0c86, 0x90c86, 0xc8c46, 0x88c46, 0xc8c46, 0x88c46, 0xc8c46, 0x88c46, 0x84826, 0x84826, 0x84826, 0x84826, 0x84826, 0x84826, 0x84426, 0x84426, 0x84426, 0x84426, 0x86426, 0x86426, 0x86026, 0x86026, ],
    3: [0x481613, 0x481613, 0x481613, 0x481613, 0x48150b, 0x48150b, 0x48150b, 0x48150b, 0x48150b, 0x48150b, 0x481487, 0x481487, 0x481487, 0x481487, 0x481487, 0x481487, 0x480487, 0x480487, 0x480487, 0x480487, 0x480487, 0x480487, 0x80447, 0x80447, 0x80447, 0x80447, 0x80447, 0x80447, 0x80427, 0x80427, 0x80427, 0x80427, 0x80427, 0x80427, 0x80427, 0x80427, 0x80427, 0x80427, 0x80427, 0x80427, 0x80027, 0x80027, ],
}


def _plan(protocol, n, rounds, c0_points, timing=0, n_simds=1024, lane_group=0):
    from emul.build_agg import load
    out = (np.zeros(10, np.uint32))
    load().emul_agg_plan(protocol, n, rounds, n_simds, timing, lane_group, c0_points, out.ctypes.data)
    return dict(zip(("code", "p1_group", "fb", "beside", "c0var_group", "c0_chunks", "round_group", "tab_parts", "final_lg", "per_point"),
                    (int(v) for v in out)))


def test_the_older_protocols_plans_are_unchanged():
    for name, p in PROTOCOL.items():
        got = [_plan(p, T * 1024 + d, SHAPE[name][0], SHAPE[name][1], timing)["code"] for T in GRID_T for d in (-1, 0, 1) for timing in (0, 1)]
        assert got == CODES_BEFORE[p], name
        assert all(c >> 23 == 0 for c in got)


def agg_expected_form(T, d, rounds):
    """The reciprocal verifier's row of tests/generic_forms.py -- the aggregate verifier takes phase 1's lanes, `beside` and the
    fixed-base form by the same sizes -- with the final scalars' lanes clipped to the rounds of the shape."""
    f = dict(FORMS[("recip", T)][d + 1], protocol="aggregate")
    f["final_scalars_lg"] = min(f["final_scalars_lg"], max(rounds - 1, 0))
    return f


def _decode(v):
    from types import SimpleNamespace
    from bp_pp_amd.wnla import WeightNormLinearArgument
    return WeightNormLinearArgument.generic_form(SimpleNamespace(get_option=lambda name: v))


def test_the_aggregate_plan_at_its_thresholds():
    S = 1024
    for T in GRID_T:
        for d in (-1, 0, 1):
            for rounds, k in ((3, 2), (6, 16)):
                p = _plan(AGGREGATE, T * S + d, rounds, 4 + k)
                assert _decode(p["code"]) == agg_expected_form(T, d, rounds), (T, d, rounds)
                assert p["code"] >> 23 == 1 and p["code"] & 3 == 0
                assert p["c0var_group"] == 1 and p["per_point"] == 0 and p["c0_chunks"] == (4 + k + 4) // 5
                assert _decode(_plan(AGGREGATE, T * S + d, rounds, 4 + k, timing=1)["code"]) == dict(agg_expected_form(T, d, rounds), beside=0)
    # phase 1's lanes change exactly at 8 S, 16 S, 32 S; the fixed-base form at 8 S and 128 S; on a smaller device at its own multiples
    for S in (1024, 256):
        g = lambda n: _plan(AGGREGATE, n, 6, 20, n_simds=S)
        assert [g(n)["p1_group"] for n in (1, 8 * S, 8 * S + 1, 16 * S, 16 * S + 1, 32 * S, 32 * S + 1, 1 << 21)] == [8, 8, 4, 4, 2, 2, 1, 1]
        assert [g(n)["fb"] for n in (1, 8 * S, 8 * S + 1, 128 * S - 1, 128 * S)] == [1, 1, 0, 0, 2]
        assert [g(n)["beside"] for n in (32 * S, 32 * S + 1)] == [1, 0]
    # the tests' switch: the smallest and the largest split at any size
    assert _plan(AGGREGATE, 70, 3, 6, lane_group=2)["p1_group"] == 2 and _plan(AGGREGATE, 70, 3, 6, lane_group=4)["p1_group"] == 8
