"""The golden aggregated reciprocal range proofs (tests/golden/agg_cases.json, written by tests/golden/make_agg_cases.py with the
oracle): per shape a few instances and the oracle's verdict on every corrupted row of agg_cases.corrupted_batch."""
import json
import os

import numpy as np

import agg_cases as A

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agg_cases.json")
_cache = {}


def load(shape):
    """-> (case, commitments [P, k, 64], proofs [P, proof_bytes], corrupted [(row, kind, accept, flagged)])"""
    if shape not in _cache:
        if "file" not in _cache:
            with open(PATH) as f:
                _cache["file"] = json.load(f)
        g = _cache["file"]["%d,%d,%d" % shape]
        case = A.setup(*shape)
        assert (g["rounds"], g["nl"], g["nn"]) == (case["rounds"], case["nl"], case["nn"])
        coms = np.frombuffer(b"".join(bytes.fromhex(c) for c in g["commitments"]), np.uint8).reshape(-1, shape[0], 64).copy()
        proofs = np.frombuffer(b"".join(bytes.fromhex(p) for p in g["proofs"]), np.uint8).reshape(len(g["proofs"]), -1).copy()
        assert proofs.shape[1] == case["proof_bytes"]
        _cache[shape] = (case, coms, proofs, [tuple(r) for r in g["corrupted"]])
    return _cache[shape]


def batch(shape):
    """The corrupted batch of agg_cases.ROWS rows and what the oracle says of every row: (case, C, Q, expect_acc, expect_flag, kinds)."""
    case, coms, proofs, corrupted = load(shape)
    C, Q, kinds = A.corrupted_batch(case, list(coms.reshape(len(coms), -1)), list(proofs))
    assert kinds == [(r, kind) for r, kind, _, _ in corrupted], "tests/golden/agg_cases.json is stale: run tests/golden/make_agg_cases.py"
    acc, flag = np.ones(A.ROWS, np.uint8), np.zeros(A.ROWS, bool)
    for r, _, a, f in corrupted:
        acc[r], flag[r] = a, bool(f)
    return case, C, Q, acc, flag, kinds


def generators(case):
    """g | g_vec || g_vec_ | h_vec || h_vec_ as the fixed-base tables take them."""
    return case["g"] + b"".join(case["gv"]) + b"".join(case["gv_"]) + b"".join(case["hv"]) + b"".join(case["hv_"])
