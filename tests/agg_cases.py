"""Seeded AGGREGATED reciprocal range-proof instances: k values under one proof, built on the oracle's generic ArithmeticCircuit
(oracle/bppp_oracle.py, unchanged).  The circuit is the reference's reciprocal `make_circuit` (reciprocal.rs:150-214) written for k
values that share one multiplicity vector:

    nv = nd + 1, nm = k nd, J = i nd + d (value i, digit d)
    dim_nm = nm, dim_no = np, k = k, dim_nv = nv, dim_nl = k nv, dim_nw = 2 nm + np, f_l, a_m = 1, a_l = 0, partition LL for index < np
    W_m[J][nm + J] = -e          W_l[i nv][i nd + d] = -np^d
    W_l[i nv + 1 + d]: 1 at every column nm + J' with J' != J, -(e + j)^-1 at column 2 nm + j (j < np)
    witness: w_l = all digits (value-major), w_r = (digit + e)^-1, w_o = multiplicities over all k nd digits, v_i = [x_i, r_i]
    transcript: app_point("reciprocal_commitment", V_i) for i < k, e = challenge("reciprocal_challenge"), then
                ArithmeticCircuit.verify([V_i + R_i], t, circuit_proof) with R_i = commit_poles(r_i, blind_i)
    proof bytes: c_l c_r c_o c_s | r[rounds] | x[rounds] | R_0 .. R_{k-1} | l[nl] | n[nn];  commitments: k x 64, value-major

With k = 1 this is ReciprocalRangeProofProtocol byte for byte (tests/test_agg_oracle.py)."""
import hashlib

import numpy as np

import bppp_oracle as O

N = O.N
FIELD_P = 2**256 - 2**32 - 977
# (k, nd, np) of the GPU test and why: tests/test_gpu_agg.py
SHAPES = [(1, 4, 4), (2, 4, 4), (3, 4, 4), (6, 2, 3), (7, 3, 4), (16, 16, 16)]


def _sc(tag: bytes, *idx) -> int:
    return O.wide_reduce(hashlib.shake_256(b"bppp-agg-cases" + tag + b"".join(int(i).to_bytes(4, "little") for i in idx)).digest(64))


def _pow2_at_least(n):
    p = 1
    while p < n:
        p *= 2
    return p


def proof_shape(NG, NH):
    """(rounds, nl, nn) of the WNLA argument over NH + NG entries (wnla.rs: halve until fewer than six are left)."""
    rounds, nl, nn = 0, NH, NG
    while nl + nn >= 6:
        nl, nn, rounds = (nl + 1) // 2, (nn + 1) // 2, rounds + 1
    return rounds, nl, nn


def proof_bytes(k, rounds, nl, nn):
    return 64 * (4 + 2 * rounds + k) + 32 * (nl + nn)


def _gen(tag, i):
    """Generator as 64 bytes: the C oracle's scalar multiplication when it is built (fast), the Python one otherwise."""
    s = _sc(b"gen" + tag, i)
    try:
        import bppp_oracle_c as OC
        return OC.point_mul(None, O.sc_to_bytes(s))
    except Exception:
        return O.pt_to_xy64(O.pt_mul(O.G, s))


def setup(k, nd, np_, label=b"aggregate test"):
    """Generators (bytes and oracle points) and sizes of one shape."""
    nm, nh = k * nd, nd + 10
    NG, NH = _pow2_at_least(nm), _pow2_at_least(nh)
    case = dict(k=k, nd=nd, np=np_, nm=nm, nv=nd + 1, nh=nh, NG=NG, NH=NH, label=label)
    case["g"] = _gen(b"g", 0)
    case["gv"] = [_gen(b"gv", i) for i in range(nm)]
    case["hv"] = [_gen(b"hv", i) for i in range(nh)]
    case["gv_"] = [_gen(b"gv_", i) for i in range(NG - nm)]
    case["hv_"] = [_gen(b"hv_", i) for i in range(NH - nh)]
    for key in ("gv", "hv", "gv_", "hv_"):
        case["P" + key] = [O.pt_from_xy64(b) for b in case[key]]
    case["Pg"] = O.pt_from_xy64(case["g"])
    case["rounds"], case["nl"], case["nn"] = proof_shape(NG, NH)
    case["proof_bytes"] = proof_bytes(k, case["rounds"], case["nl"], case["nn"])
    return case


def make_circuit(case, e):
    k, nd, np_, nm, nv = case["k"], case["nd"], case["np"], case["nm"], case["nv"]
    nl, nw = k * nv, 2 * nm + np_
    W_m = [[0] * nw for _ in range(nm)]
    for J in range(nm):
        W_m[J][nm + J] = O.minus(e)
    W_l = [[0] * nw for _ in range(nl)]
    inv = [O.minus(O.sc_inv((e + j) % N)) for j in range(np_)]
    for i in range(k):
        for d in range(nd):
            W_l[i * nv][i * nd + d] = O.minus(O.sc_pow(np_ % N, d))
            row = W_l[i * nv + 1 + d]
            for J in range(nm):
                row[nm + J] = 1
            row[nm + i * nd + d] = 0
            for j in range(np_):
                row[2 * nm + j] = inv[j]

    def partition(typ, index):
        return index if typ == O.LL and index < np_ else None

    return O.ArithmeticCircuit(dim_nm=nm, dim_no=np_, k=k, dim_nl=nl, dim_nv=nv, dim_nw=nw, g=case["Pg"], g_vec=list(case["Pgv"]),
                               h_vec=list(case["Phv"]), W_m=W_m, W_l=W_l, a_m=[1] * nm, a_l=[0] * nl, f_l=True, f_m=False,
                               g_vec_=list(case["Pgv_"]), h_vec_=list(case["Phv_"]), partition=partition)


def seeded_digits(case, b):
    """Digits of instance b, value-major; instance 0 is all zeros and instance 1 all np - 1 (the range's two ends)."""
    k, nd, np_ = case["k"], case["nd"], case["np"]
    if b == 0:
        return [[0] * nd for _ in range(k)]
    if b == 1:
        return [[np_ - 1] * nd for _ in range(k)]
    return [[_sc(b"digit", b, i, d) % np_ for d in range(nd)] for i in range(k)]


def value_commitment(case, x, s):
    return O.pt_add(O.pt_mul(case["Pg"], x % N), O.pt_mul(case["Phv"][0], s % N))


def prove(case, b, digits=None, xs=None, claimed=None):
    """Instance b -> (commitments k x 64 bytes, proof bytes).  digits: the digits the reciprocals are made from (default: seeded);
    xs: the committed values (default: what the digits spell); claimed: the digits put into w_l (default: `digits`) -- the last
    two let a test build dishonest witnesses."""
    k, nd, np_ = case["k"], case["nd"], case["np"]
    digits = digits if digits is not None else seeded_digits(case, b)
    claimed = claimed if claimed is not None else digits
    xs = xs if xs is not None else [sum(dg * np_**d for d, dg in enumerate(row)) for row in digits]
    ss = [_sc(b"s", b, i) for i in range(k)]
    V = [value_commitment(case, xs[i], ss[i]) for i in range(k)]
    flat = [d for row in claimed for d in row]
    m = [flat.count(v) for v in range(np_)]
    cnt = [0]

    def rng():
        cnt[0] += 1
        return _sc(b"rnd", b, cnt[0])

    t = O.Transcript(case["label"])
    for v in V:
        O.app_point(b"reciprocal_commitment", v, t)
    e = O.get_challenge(b"reciprocal_challenge", t)
    r = [[O.sc_inv((d + e) % N) for d in row] for row in digits]
    rb = [rng() for _ in range(k)]
    R = [O.pt_add(O.pt_mul(case["Phv"][0], rb[i]), O.vector_mul(case["Phv"][9:], r[i], O.PT)) for i in range(k)]
    circ = make_circuit(case, e)
    cw = O.CircuitWitness(v=[[xs[i] % N] + r[i] for i in range(k)], s_v=[(ss[i] + rb[i]) % N for i in range(k)], w_l=flat,
                          w_r=[a for row in r for a in row], w_o=m)
    p = circ.prove([O.pt_add(V[i], R[i]) for i in range(k)], cw, t, rng)
    assert (len(p.r), len(p.l), len(p.n)) == (case["rounds"], case["nl"], case["nn"])
    blob = b"".join(O.pt_to_xy64(q) for q in [p.c_l, p.c_r, p.c_o, p.c_s] + list(p.r) + list(p.x) + R)
    blob += b"".join(O.sc_to_bytes(v) for v in list(p.l) + list(p.n))
    assert len(blob) == case["proof_bytes"]
    return b"".join(O.pt_to_xy64(v) for v in V), blob


def verify(case, commitments: bytes, proof: bytes, trace=None) -> int:
    """1 accept, 0 reject, -1 an input k256 would not have deserialised, -2 a degenerate challenge or a zero inverse."""
    k, rounds, nl, nn = case["k"], case["rounds"], case["nl"], case["nn"]
    try:
        V = [O.pt_from_xy64(commitments[64 * i:64 * i + 64]) for i in range(k)]
        npts = 4 + 2 * rounds + k
        pts = [O.pt_from_xy64(proof[64 * i:64 * i + 64]) for i in range(npts)]
        for c in list(commitments[j:j + 32] for j in range(0, 64 * k, 32)) + [proof[j:j + 32] for j in range(0, 64 * npts, 32)]:
            if int.from_bytes(c, "big") >= FIELD_P:
                return -1
        scal = [O.sc_from_bytes(proof[64 * npts + 32 * i:64 * npts + 32 * i + 32]) for i in range(nl + nn)]
    except ValueError:
        return -1
    R = pts[4 + 2 * rounds:]
    cp = O.CircuitProof(c_l=pts[0], c_r=pts[1], c_o=pts[2], c_s=pts[3], r=pts[4:4 + rounds], x=pts[4 + rounds:4 + 2 * rounds],
                        l=scal[:nl], n=scal[nl:])
    try:
        t = O.Transcript(case["label"])
        for v in V:
            O.app_point(b"reciprocal_commitment", v, t)
        e = O.get_challenge(b"reciprocal_challenge", t)
        sums = [O.pt_add(V[i], R[i]) for i in range(k)]
        if trace is not None:
            trace.extend([("e", e), ("V+R", sums)])
        return 1 if make_circuit(case, e).verify(sums, t, cp, trace) else 0
    except (O.DegenerateChallenge, ZeroDivisionError):
        return -2


def neg_point(xy: bytes) -> bytes:
    y = int.from_bytes(xy[32:], "big")
    return bytes(xy[:32]) + ((FIELD_P - y) % FIELD_P).to_bytes(32, "big")


# ---- the corrupted batch of the GPU test: ROWS instances replicated from a few oracle proofs, one row per field class
ROWS = 70


def field_offsets(case):
    """Byte offset in the proof of each field class the GPU test corrupts."""
    k, rounds, nl = case["k"], case["rounds"], case["nl"]
    R0 = 64 * (4 + 2 * rounds)
    sc0 = R0 + 64 * k
    return dict(c_l=0, c_r=64, c_o=128, c_s=192, r=256 + 64 * (rounds - 1), x=256 + 64 * rounds, R_first=R0, R_mid=R0 + 64 * (k // 2),
                R_last=R0 + 64 * (k - 1), l=sc0, n=sc0 + 32 * nl)


def corrupted_batch(case, coms, proofs):
    """(commitments [ROWS, k, 64], proofs [ROWS, proof_bytes], [(row, kind)]): row i starts as pool entry i mod len(pool); then one
    row per field class is corrupted in place.  Deterministic: the golden file's expectations are for exactly this batch."""
    k = case["k"]
    P = len(proofs)
    idx = np.arange(ROWS) % P
    C = np.ascontiguousarray(np.frombuffer(b"".join(bytes(c) for c in coms), np.uint8).reshape(P, k, 64)[idx])
    Q = np.ascontiguousarray(np.frombuffer(b"".join(bytes(p) for p in proofs), np.uint8).reshape(P, -1)[idx])
    off = field_offsets(case)
    kinds = []
    row = 3
    for name in ("c_l", "c_r", "c_o", "c_s", "r", "x", "R_first", "R_mid", "R_last"):      # a valid but wrong point: another field's
        o, other = off[name], off["c_s" if name != "c_s" else "c_l"]
        Q[row, o:o + 64] = Q[row, other:other + 64].copy()
        kinds.append((row, name)); row += 3
    for name in ("l", "n"):                                                                # a low bit: the scalar stays canonical
        Q[row, off[name] + 31] ^= 1
        kinds.append((row, name)); row += 3
    C[row, 0] = C[(row + 1) % ROWS, 0] if P > 1 else np.frombuffer(neg_point(C[row, 0].tobytes()), np.uint8)
    kinds.append((row, "V_first")); row += 3
    C[row, k - 1] = np.frombuffer(neg_point(C[row, k - 1].tobytes()), np.uint8)
    kinds.append((row, "V_last")); row += 3
    if k > 1:
        C[row, [0, 1]] = C[row, [1, 0]]
        kinds.append((row, "V_swapped")); row += 3
    Q[row, off["R_mid"] + 40] ^= 1                                                         # off the curve: the status bit
    kinds.append((row, "R_off_curve")); row += 3
    C[row, k - 1, 63] ^= 1
    kinds.append((row, "V_off_curve")); row += 3
    Q[row, off["c_o"]:off["c_o"] + 32] = np.frombuffer(FIELD_P.to_bytes(32, "big"), np.uint8)
    kinds.append((row, "coordinate_p")); row += 3
    o = off["R_last"]
    C[row, k - 1] = Q[row, o:o + 64]                                                       # V_i = R_i: the doubling case of the sum
    kinds.append((row, "V_eq_R")); row += 3
    C[row, 0] = np.frombuffer(neg_point(Q[row, off["R_first"]:off["R_first"] + 64].tobytes()), np.uint8)   # V_i = -R_i: the identity
    kinds.append((row, "V_eq_negR")); row += 3
    Q[ROWS - 1, off["n"] + 30] ^= 4                                                        # the last row: what a short grid drops
    kinds.append((ROWS - 1, "n_last_row"))
    assert row < ROWS - 1
    return C, Q, kinds


def expectations(case, C, Q, kinds):
    """The oracle's (accept, flagged) on every corrupted row."""
    out = {}
    for row, kind in kinds:
        rc = verify(case, C[row].tobytes(), Q[row].tobytes())
        out[row] = (1 if rc == 1 else 0, rc < 0)
    return out
