"""Writes tests/golden/agg_cases.json: for every shape of tests/agg_cases.py SHAPES a few aggregated reciprocal range proofs made by
the Python oracle (the (16, 16, 16) ones take ten seconds each), and the oracle's verdict on every corrupted row of the batch
agg_cases.corrupted_batch builds from them -- so the GPU test spends no time in the oracle.  tests/test_agg_oracle.py re-derives part
of the file on the CPU.  Run from the repository root:  python tests/golden/make_agg_cases.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import agg_cases as A  # noqa: E402

POOL = {(16, 16, 16): 3}       # instances per shape (default 5)


def main():
    out = {}
    for shape in A.SHAPES:
        case = A.setup(*shape)
        P = POOL.get(shape, 5)
        made = [A.prove(case, b) for b in range(P)]
        assert all(A.verify(case, c, p) == 1 for c, p in made), shape
        C, Q, kinds = A.corrupted_batch(case, [c for c, _ in made], [p for _, p in made])
        exp = A.expectations(case, C, Q, kinds)
        out["%d,%d,%d" % shape] = dict(rounds=case["rounds"], nl=case["nl"], nn=case["nn"], commitments=[c.hex() for c, _ in made],
                                       proofs=[p.hex() for _, p in made],
                                       corrupted=[[row, kind, exp[row][0], int(exp[row][1])] for row, kind in kinds])
        print(shape, "done", flush=True)
    with open(os.path.join(HERE, "agg_cases.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
