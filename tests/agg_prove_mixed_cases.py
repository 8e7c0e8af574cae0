"""Inputs and expected outputs of the aggregated reciprocal PROVER for mixed value counts (bppp_reciprocal_agg_prove_values_batch_mixed*),
from what is already stored: tests/golden/agg_mixed_cases.json holds, per context shape (k_max, nd, np) and value count k, oracle proofs
made by agg_cases.prove(setup_on(case_max, k), 10 k + j) on the k_max context's generators; agg_prove_cases.inputs rebuilds the x, s and
draws that the oracle was fed.  build() lays both out by k_max, as the mixed calls take and give them."""
import numpy as np

import agg_mixed_cases as M
import agg_prove_cases as AP

_inputs = {}


def draws(k, nd):
    return k + 18 + (nd + 1) + k * nd


def pool_inputs(shape, k, j):
    """(x [k, 32], s [k, 32], rnd [draws(k), 32]) of pool proof j of value count k; made once, read-only."""
    key = (shape, k, j)
    if key not in _inputs:
        case_max, _ = M.load_pool(shape)
        arrs = AP.inputs(M.setup_on(case_max, k), 10 * k + j, draws(k, shape[1]))
        for a in arrs:
            a.setflags(write=False)
        _inputs[key] = arrs
    return _inputs[key]


def cycle(shape, n, start=0):
    """n value counts cycling through the shape's, so that neighbours differ."""
    KS = M.CONTEXTS[shape]
    return [KS[(start + i) % len(KS)] for i in range(n)]


def build(shape, ks, fill=0xFF):
    """ks -> (x [n, k_max, 32], s, rnd [n, draws(k_max), 32], C [n, k_max, 64], Q [n, proof_bytes(k_max)]): inputs with `fill` in every
    unused slot, and the expected outputs: the pool's bytes, zero behind them.  Row t takes pool proof (rows of its count before t) mod
    the pool's size."""
    case_max, pool = M.load_pool(shape)
    k_max, nd = shape[0], shape[1]
    n = len(ks)
    x = np.full((n, k_max, 32), fill, np.uint8)
    s = np.full((n, k_max, 32), fill, np.uint8)
    rnd = np.full((n, draws(k_max, nd), 32), fill, np.uint8)
    C = np.zeros((n, k_max, 64), np.uint8)
    Q = np.zeros((n, case_max["proof_bytes"]), np.uint8)
    seen = {}
    for t, k in enumerate(ks):
        j = seen.get(k, 0) % len(pool[k])
        seen[k] = seen.get(k, 0) + 1
        xi, si, ri = pool_inputs(shape, k, j)
        x[t, :k], s[t, :k], rnd[t, :len(ri)] = xi, si, ri
        com, proof = pool[k][j]
        C[t, :k] = np.frombuffer(com, np.uint8).reshape(k, 64)
        Q[t, :len(proof)] = np.frombuffer(proof, np.uint8)
    return x, s, rnd, C, Q
