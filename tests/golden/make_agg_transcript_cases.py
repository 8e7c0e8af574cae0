"""Writes tests/golden/agg_transcript_cases.json: for every shape of tests/agg_transcript_cases.py SHAPES aggregated reciprocal range
proofs made by the Python oracle ON PRE-LOADED TRANSCRIPTS -- one per sponge position of the mixed batch, and a few on one shared
state -- with the state the oracle's prover leaves, and the oracle's verdict and advanced state on one corrupted row per field class,
so the GPU test spends no time in the oracle.  tests/test_agg_transcript_oracle.py re-derives part of the file on the CPU.
Run from the repository root:  python tests/golden/make_agg_transcript_cases.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), ROOT]

import agg_cases as A  # noqa: E402
import agg_transcript_cases as AT  # noqa: E402


def entry(case, state, b):
    c, p, out = AT.prove_state(case, state, b)
    acc, flagged, vout = AT.verify_state(case, state, c, p)
    assert acc == 1 and not flagged and vout == out, (b, "the verifier must reach the prover's state")
    return dict(b=b, commitments=c.hex(), proof=p.hex(), state_out=out.hex())


def main():
    out = {}
    for shape in AT.SHAPES:
        case = A.setup(*shape)
        npos = len(AT.mixed_positions(case["label"]))
        mixed = [entry(case, AT.mixed_state(case, b), b) for b in range(npos)]
        shared = [entry(case, AT.shared_state(case), npos + j) for j in range(AT.SHARED_POOL.get(shape, 2))]
        corrupted = []
        for i, kind in enumerate(AT.CLASSES):
            C = np.frombuffer(bytes.fromhex(mixed[i]["commitments"]), np.uint8).reshape(shape[0], 64).copy()
            Q = np.frombuffer(bytes.fromhex(mixed[i]["proof"]), np.uint8).copy()
            AT.corrupt(case, C, Q, kind)
            acc, flagged, sout = AT.verify_state(case, AT.mixed_state(case, i), C.tobytes(), Q.tobytes())
            corrupted.append([i, kind, acc, int(flagged), sout.hex()])
        # a proof bound to one transcript under another: entry 0's proof on entry 1's state
        acc, flagged, sout = AT.verify_state(case, AT.mixed_state(case, 1), bytes.fromhex(mixed[0]["commitments"]), bytes.fromhex(mixed[0]["proof"]))
        out["%d,%d,%d" % shape] = dict(rounds=case["rounds"], nl=case["nl"], nn=case["nn"], mixed=mixed, shared=shared, corrupted=corrupted,
                                       rebound=[acc, int(flagged), sout.hex()])
        print(shape, "done", flush=True)
    with open(os.path.join(HERE, "agg_transcript_cases.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
