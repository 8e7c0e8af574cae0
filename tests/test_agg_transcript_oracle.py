"""tests/golden/agg_transcript_cases.json against the oracle it was made from (tests/agg_transcript_cases.py), on the CPU: per shape
one entry of the mixed pool is proved again on its pre-loaded transcript and must give the file's bytes and state, the verifier must
reach the prover's state, and one corrupted row must get the file's verdict.  The (16, 16, 16) shape is re-verified, not re-proved
(its proofs take ten seconds each).  Also what the helpers promise about sponge positions."""
import json
import os

import numpy as np
import pytest

import agg_cases as A
import agg_transcript_cases as AT
import bppp_oracle as O

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_transcript_cases.json")


@pytest.fixture(scope="module")
def golden():
    with open(PATH) as f:
        return json.load(f)


def test_positions_of_the_mixed_batch():
    label = A.setup(2, 4, 4)["label"]
    pos = AT.mixed_positions(label)
    assert len(set(pos)) == 6 and pos[0] == AT.lowest_position(label) == 0 and 165 in pos
    assert sum(140 <= p <= 163 for p in pos) >= 2 and sum(104 <= p <= 136 for p in pos) >= 2
    for b, p in enumerate(pos):
        s = AT.state_at(label, p, salt=b)
        assert len(s) == 203 and s[200] == p and s[201] <= AT.RATE and AT.ser(AT.unser(s)) == s
    # the rate boundary really is where the docstring puts it: from 150 the meta-AD wraps, from 120 the data does
    for p, where in ((150, "meta"), (120, "data")):
        t = AT.unser(AT.state_at(label, p))
        t.strobe.meta_ad(b"reciprocal_commitment", False)
        t.strobe.meta_ad((33).to_bytes(4, "little"), True)
        wrapped_in_meta = t.strobe.pos < p
        assert wrapped_in_meta == (where == "meta"), (p, t.strobe.pos)


@pytest.mark.parametrize("shape", AT.SHAPES)
def test_golden_entries_recomputed(golden, shape):
    g = golden["%d,%d,%d" % shape]
    case = A.setup(*shape)
    assert (g["rounds"], g["nl"], g["nn"]) == (case["rounds"], case["nl"], case["nn"])
    i = 2
    e = g["mixed"][i]
    state = AT.mixed_state(case, i)
    c, p, out = bytes.fromhex(e["commitments"]), bytes.fromhex(e["proof"]), bytes.fromhex(e["state_out"])
    if shape[0] < 16:
        assert AT.prove_state(case, state, e["b"]) == (c, p, out)
    assert AT.verify_state(case, state, c, p) == (1, False, out)
    if shape[0] < 16:
        entry, kind, acc, flagged, sout = g["corrupted"][3]
        C = np.frombuffer(bytes.fromhex(g["mixed"][entry]["commitments"]), np.uint8).reshape(shape[0], 64).copy()
        Q = np.frombuffer(bytes.fromhex(g["mixed"][entry]["proof"]), np.uint8).copy()
        AT.corrupt(case, C, Q, kind)
        st = AT.mixed_state(case, entry)
        assert AT.verify_state(case, st, C.tobytes(), Q.tobytes()) == (acc, bool(flagged), bytes.fromhex(sout)) == (0, True, st)


def test_on_the_label_state_it_is_agg_cases():
    """The restated transcript on Transcript::new(label) is agg_cases.prove / verify byte for byte."""
    case = A.setup(2, 4, 4)
    c, p = A.prove(case, 3)
    t = O.Transcript(case["label"])
    assert AT.prove_on(case, t, 3) == (c, p)
    assert AT.verify_on(case, O.Transcript(case["label"]), c, p) == A.verify(case, c, p) == 1
