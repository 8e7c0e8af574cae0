"""Writes tests/golden/agg_mixed_cases.json: for every context shape of tests/agg_mixed_cases.py CONTEXTS a few aggregated reciprocal
range proofs per value count, made by the Python oracle on the CONTEXT's generators (agg_mixed_cases.setup_on), and the oracle's
verdict on every row of the batch agg_mixed_cases.build_batch makes from them -- so the GPU test spends no time in the oracle.
tests/test_agg_mixed_oracle.py re-derives part of the file on the CPU.  The proofs and the rows are spread over worker processes (the
(16, 16, 16) ones take ten seconds each).  Run from the repository root:  python tests/golden/make_agg_mixed_cases.py"""
import json
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import agg_cases as A  # noqa: E402
import agg_mixed_cases as M  # noqa: E402


def seed_of(shape, k, j):
    """The instance number handed to agg_cases.prove: distinct per (k, j) and never 0 or 1 (the all-zero and all-maximal digits)."""
    return 10 * k + j


def _prove(job):
    shape, k, j = job
    case = M.setup_on(A.setup(*shape), k)
    com, proof = A.prove(case, seed_of(shape, k, j))
    assert A.verify(case, com, proof) == 1, job
    return job, com.hex(), proof.hex()


def _verdict(job):
    shape, row, k, com, proof = job
    rc = A.verify(M.setup_on(A.setup(*shape), k), com, proof)
    return shape, row, 1 if rc == 1 else 0, int(rc < 0)


def main():
    out = {}
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as mp:
        jobs = [(shape, k, j) for shape, KS in M.CONTEXTS.items() for k in KS for j in range(M.pool_size(shape))]
        pools = {shape: {k: [None] * M.pool_size(shape) for k in KS} for shape, KS in M.CONTEXTS.items()}
        for (shape, k, j), com, proof in mp.imap_unordered(_prove, jobs):
            pools[shape][k][j] = (com, proof)
        print("proofs done", flush=True)
        rows, batches = [], {}
        for shape in M.CONTEXTS:
            case_max = A.setup(*shape)
            pool = {k: [(bytes.fromhex(c), bytes.fromhex(p)) for c, p in v] for k, v in pools[shape].items()}
            ks, C, Q, notes = M.build_batch(shape, pool)
            batches[shape] = (ks, notes)
            for row in range(M.ROWS):
                case, com, proof = M.row_inputs(case_max, ks, C, Q, row)
                rows.append((shape, row, case["k"], com, proof))
        verdicts = {shape: [None] * M.ROWS for shape in M.CONTEXTS}
        for shape, row, acc, flag in mp.imap_unordered(_verdict, rows, chunksize=4):
            verdicts[shape][row] = (acc, flag)
    for shape in M.CONTEXTS:
        case_max = A.setup(*shape)
        ks, notes = batches[shape]
        noted = dict(notes)
        assert all(verdicts[shape][r] == (1, 0) for r in range(M.CLEAN)), shape
        for r in range(M.ROWS):
            if r in noted and noted[r] in ("unused_ff", "unused_other"):
                assert verdicts[shape][r] == (1, 0), (shape, r)
        out["%d,%d,%d" % shape] = dict(rounds=case_max["rounds"], nl=case_max["nl"], nn=case_max["nn"],
                                       pool={str(k): [list(e) for e in v] for k, v in pools[shape].items()},
                                       rows=[[int(ks[r]), verdicts[shape][r][0], verdicts[shape][r][1], noted.get(r, "clean")]
                                             for r in range(M.ROWS)])
        print(shape, "done", flush=True)
    with open(os.path.join(HERE, "agg_mixed_cases.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
