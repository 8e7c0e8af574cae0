"""Inputs of the aggregated reciprocal PROVER for the golden instances of tests/golden/agg_cases.json: the integers x_i, the blindings
s_i and the draws `rnd` that tests/agg_cases.py::prove fed the oracle's prover for instance b, rebuilt from the same seeded functions
-- so that a prover under test is compared with the golden bytes and no test spends time in the Python oracle's prover."""
import numpy as np

import agg_cases as A

N = A.N


def be32(v: int) -> bytes:
    return int(v).to_bytes(32, "big")


def inputs(case, b, draws: int):
    """Instance b -> (x [k, 32], s [k, 32], rnd [draws, 32]) as uint8 arrays.  draws: what the library under test says it takes per
    instance (bppp_reciprocal_agg_prove_draws(k, nd)); it must be what the oracle's prover drew: rb_0 .. rb_{k-1}, then
    ArithmeticCircuit.prove's 18 + dim_nv + dim_nm."""
    k, nd, np_ = case["k"], case["nd"], case["np"]
    assert draws == k + 18 + (nd + 1) + k * nd, (draws, k, nd)
    digits = A.seeded_digits(case, b)
    xs = [sum(dg * np_**d for d, dg in enumerate(row)) for row in digits]
    ss = [A._sc(b"s", b, i) for i in range(k)]
    rnd = [A._sc(b"rnd", b, j) for j in range(1, draws + 1)]
    assert len(rnd) == draws
    arr = lambda vals: np.frombuffer(b"".join(be32(v) for v in vals), np.uint8).reshape(len(vals), 32).copy()
    return arr(xs), arr(ss), arr(rnd)


def batch(case, bs, draws: int):
    """Instances bs -> (x [B, k, 32], s [B, k, 32], rnd [B, draws, 32])."""
    rows = [inputs(case, b, draws) for b in bs]
    return tuple(np.ascontiguousarray(np.stack([r[i] for r in rows])) for i in range(3))


def digits_and_counts(x: int, nd: int, np_: int):
    """The low nd base-np digits of x (least significant first) and what is left above them."""
    out = []
    for _ in range(nd):
        out.append(x % np_)
        x //= np_
    return out, x
