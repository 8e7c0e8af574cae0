"""CPU checks of the mixed-value-count fixture (tests/agg_mixed_cases.py, tests/golden/agg_mixed_cases.json) against the in-repo
oracle: the golden file is the batch the builder makes today, a case on the context's generators with k = k_max is the context's own
case, part of the recorded verdicts is re-derived, and a proof made for one value count is not a proof for another."""
import numpy as np
import pytest

import agg_cases as A
import agg_mixed_cases as M

SMALL = [s for s in M.CONTEXTS if s != (16, 16, 16)]


@pytest.mark.parametrize("shape", list(M.CONTEXTS))
def test_the_golden_file_is_the_builders_batch(shape):
    case_max, ks, C, Q, acc, flag, notes = M.batch(shape)
    KS = M.CONTEXTS[shape]
    assert len(ks) == M.ROWS and 65 <= M.ROWS <= 75 and set(ks.tolist()) <= set(KS) | {KS[0] + 1, KS[-1] - 1}
    assert ks[:len(KS)].tolist() == KS and all(ks[i] != ks[i + 1] for i in range(M.CLEAN - 1))      # neighbouring lanes differ
    assert acc[:M.CLEAN].all() and not flag[:M.CLEAN].any()
    noted = dict(notes)
    kinds = {what.split(",")[0] for what in noted.values()}
    assert kinds == set(M.KINDS) | {"unused_ff", "unused_other", "wrong_k_plus", "wrong_k_minus", "n_last_row"}
    for kind in M.KINDS:                          # every field class on the smallest and on the largest value count
        assert {"%s,k=%d" % (kind, KS[0]), "%s,k=%d" % (kind, KS[-1])} <= set(noted.values())
    assert not acc[[r for r, what in notes if what.split(",")[0] in M.KINDS]].any()
    stride = A.proof_bytes(shape[0], case_max["rounds"], case_max["nl"], case_max["nn"])
    assert Q.shape == (M.ROWS, stride) and C.shape == (M.ROWS, shape[0], 64)


def test_setup_on_with_k_max_is_the_contexts_own_case_and_smaller_k_shares_its_generators():
    for shape in SMALL:
        case_max = A.setup(*shape)
        same = M.setup_on(case_max, shape[0])
        assert all(same[key] == case_max[key] for key in case_max)
        for k in M.CONTEXTS[shape]:
            c = M.setup_on(case_max, k)
            assert c["gv"] + c["gv_"] == case_max["gv"] + case_max["gv_"] and len(c["gv"]) == k * shape[1]
            assert (c["hv"], c["hv_"], c["NG"], c["NH"]) == (case_max["hv"], case_max["hv_"], case_max["NG"], case_max["NH"])
            assert (c["rounds"], c["nl"], c["nn"]) == (case_max["rounds"], case_max["nl"], case_max["nn"])


@pytest.mark.parametrize("shape", [(3, 4, 4), (6, 2, 3)])
def test_recorded_verdicts_are_the_oracles(shape):
    """Re-derived here: a clean row of every value count, the rows about unused slot bytes and wrong counts, and every sixth
    corrupted row."""
    case_max, ks, C, Q, acc, flag, notes = M.batch(shape)
    rows = list(range(len(M.CONTEXTS[shape]))) + list(range(M.CLEAN, M.ROWS - 5, 6)) + list(range(M.ROWS - 5, M.ROWS))
    for r in rows:
        case, com, proof = M.row_inputs(case_max, ks, C, Q, r)
        rc = A.verify(case, com, proof)
        assert (1 if rc == 1 else 0, rc < 0) == (int(acc[r]), bool(flag[r])), (shape, r, dict(notes).get(r, "clean"))


def test_a_proof_for_k_values_is_no_proof_for_another_count_on_the_same_context():
    shape = (3, 4, 4)
    case_max, pool = M.load_pool(shape)
    com2, proof2 = pool[2][0]
    assert A.verify(M.setup_on(case_max, 2), com2, proof2) == 1
    # read as one value: R_1 sits where l is looked for; read as three: the scalars and zero bytes stand in for R_2
    pb1 = A.proof_bytes(1, case_max["rounds"], case_max["nl"], case_max["nn"])
    assert A.verify(M.setup_on(case_max, 1), com2[:64], proof2[:pb1]) != 1
    pad = proof2 + bytes(case_max["proof_bytes"] - len(proof2))
    assert A.verify(M.setup_on(case_max, 3), com2 + bytes(64), pad) != 1
    # and the golden proofs of tests/golden/agg_cases.json for k = 2 sit on other padding generators: no use on this context
    import agg_golden
    _, coms, proofs, _ = agg_golden.load((2, 4, 4))
    assert A.verify(M.setup_on(case_max, 2), coms[0].tobytes(), proofs[0].tobytes()) != 1
