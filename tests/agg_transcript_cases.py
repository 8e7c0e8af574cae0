"""Aggregated reciprocal range proofs on PRE-LOADED transcripts, stated on the oracle: the transcript of agg_cases.verify / agg_cases.prove
restated so that it takes an O.Transcript the caller has already appended to (the reference's `t: &mut Transcript`), and helpers that
build such transcripts at chosen sponge positions and read the advanced state back.  Circuits, generators, digits and draws are
agg_cases' own.

A pre-loaded transcript here is Transcript::new(case label) + append_message(b"ctx", <msg>): the length of msg sets the sponge position.
From position p the first app_point("reciprocal_commitment", V_0) absorbs 2 bytes (begin_op) + 25 of meta-AD (the 21-byte label and the
4-byte length) + 2 (begin_op) + 33 data bytes; the sponge's rate is 166, so
    p in [140, 163]   the append crosses the rate boundary inside its meta-AD
    p in [104, 136]   it crosses inside its 33 data bytes
POSITIONS lists what the GPU test mixes inside one wavefront."""
import numpy as np

import agg_cases as A
import bppp_oracle as O

N = O.N
RATE = 166
ST_BAD_ENCODING, ST_DEGENERATE, ST_OUT_OF_RANGE = 1, 2, 4


def ser(t: "O.Transcript") -> bytes:
    """merlin's STROBE-128 state as the 203 bytes the C ABI exchanges (transcript_cases.ser)."""
    return bytes(t.strobe.state) + bytes([t.strobe.pos, t.strobe.pos_begin, t.strobe.cur_flags])


def unser(state: bytes) -> "O.Transcript":
    t = O.Transcript(b"x")
    t.strobe.state = bytearray(state[:200])
    t.strobe.pos, t.strobe.pos_begin, t.strobe.cur_flags = state[200], state[201], state[202]
    return t


def preloaded(label: bytes, msg_len: int, salt: int = 0) -> bytes:
    """State of Transcript::new(label) after append_message(b"ctx", msg) with a msg of msg_len bytes that depends on salt."""
    t = O.Transcript(label)
    t.append_message(b"ctx", bytes((salt * 131 + 7 * i + 1) & 0xFF for i in range(msg_len)))
    return ser(t)


_pos_cache = {}


def positions_by_length(label: bytes):
    """{sponge position: shortest msg_len that leaves the pre-loaded transcript there} over msg_len < 2 * RATE."""
    if label not in _pos_cache:
        out = {}
        for n in range(2 * RATE):
            out.setdefault(preloaded(label, n)[200], n)
        _pos_cache[label] = out
    return _pos_cache[label]


def lowest_position(label: bytes) -> int:
    return min(positions_by_length(label))


def mixed_positions(label: bytes):
    """The positions the mixed batch cycles through, neighbouring rows differing: the lowest a pre-loaded state can have, 165, two at
    which the first reciprocal_commitment append crosses the rate boundary in its meta-AD, two at which it crosses in its data bytes."""
    return [lowest_position(label), 165, 150, 120, 163, 136]


def state_at(label: bytes, pos: int, salt: int = 0) -> bytes:
    s = preloaded(label, positions_by_length(label)[pos], salt)
    assert s[200] == pos
    return s


# ---- agg_cases.verify (agg_cases.py:154-180) on the caller's transcript
def verify_on(case, t: "O.Transcript", commitments: bytes, proof: bytes, trace=None) -> int:
    """1 accept, 0 reject, -1 an input k256 would not have deserialised (t untouched), -2 a degenerate challenge or a zero inverse."""
    k, rounds, nl, nn = case["k"], case["rounds"], case["nl"], case["nn"]
    try:
        V = [O.pt_from_xy64(commitments[64 * i:64 * i + 64]) for i in range(k)]
        npts = 4 + 2 * rounds + k
        pts = [O.pt_from_xy64(proof[64 * i:64 * i + 64]) for i in range(npts)]
        for c in list(commitments[j:j + 32] for j in range(0, 64 * k, 32)) + [proof[j:j + 32] for j in range(0, 64 * npts, 32)]:
            if int.from_bytes(c, "big") >= A.FIELD_P:
                return -1
        scal = [O.sc_from_bytes(proof[64 * npts + 32 * i:64 * npts + 32 * i + 32]) for i in range(nl + nn)]
    except ValueError:
        return -1
    R = pts[4 + 2 * rounds:]
    cp = O.CircuitProof(c_l=pts[0], c_r=pts[1], c_o=pts[2], c_s=pts[3], r=pts[4:4 + rounds], x=pts[4 + rounds:4 + 2 * rounds],
                        l=scal[:nl], n=scal[nl:])
    try:
        for v in V:
            O.app_point(b"reciprocal_commitment", v, t)
        e = O.get_challenge(b"reciprocal_challenge", t)
        sums = [O.pt_add(V[i], R[i]) for i in range(k)]
        if trace is not None:
            trace.extend([("e", e), ("V+R", sums)])
        return 1 if A.make_circuit(case, e).verify(sums, t, cp, trace) else 0
    except (O.DegenerateChallenge, ZeroDivisionError):
        return -2


def verify_state(case, state: bytes, commitments: bytes, proof: bytes, trace=None):
    """-> (accept, flagged, state_out): what a `_transcript` verifier must return for this row.  A row k256 would not have deserialised
    gets its input state back."""
    t = unser(state)
    rc = verify_on(case, t, commitments, proof, trace)
    return (1 if rc == 1 else 0), rc < 0, (bytes(state) if rc == -1 else ser(t))


# ---- agg_cases.prove (agg_cases.py:118-151) on the caller's transcript, honest witnesses only
def prove_on(case, t: "O.Transcript", b: int):
    """Instance b of agg_cases (its digits, blindings and draws) proved on t -> (commitments k x 64 bytes, proof bytes); t advances."""
    k, nd, np_ = case["k"], case["nd"], case["np"]
    digits = A.seeded_digits(case, b)
    xs = [sum(dg * np_**d for d, dg in enumerate(row)) for row in digits]
    ss = [A._sc(b"s", b, i) for i in range(k)]
    V = [A.value_commitment(case, xs[i], ss[i]) for i in range(k)]
    flat = [d for row in digits for d in row]
    m = [flat.count(v) for v in range(np_)]
    cnt = [0]

    def rng():
        cnt[0] += 1
        return A._sc(b"rnd", b, cnt[0])

    for v in V:
        O.app_point(b"reciprocal_commitment", v, t)
    e = O.get_challenge(b"reciprocal_challenge", t)
    r = [[O.sc_inv((d + e) % N) for d in row] for row in digits]
    rb = [rng() for _ in range(k)]
    R = [O.pt_add(O.pt_mul(case["Phv"][0], rb[i]), O.vector_mul(case["Phv"][9:], r[i], O.PT)) for i in range(k)]
    circ = A.make_circuit(case, e)
    cw = O.CircuitWitness(v=[[xs[i] % N] + r[i] for i in range(k)], s_v=[(ss[i] + rb[i]) % N for i in range(k)], w_l=flat,
                          w_r=[a for row in r for a in row], w_o=m)
    p = circ.prove([O.pt_add(V[i], R[i]) for i in range(k)], cw, t, rng)
    blob = b"".join(O.pt_to_xy64(q) for q in [p.c_l, p.c_r, p.c_o, p.c_s] + list(p.r) + list(p.x) + R)
    blob += b"".join(O.sc_to_bytes(v) for v in list(p.l) + list(p.n))
    assert len(blob) == case["proof_bytes"]
    return b"".join(O.pt_to_xy64(v) for v in V), blob


def prove_state(case, state: bytes, b: int):
    """-> (commitments, proof, state_out) of the oracle's prove of instance b on the pre-loaded state."""
    t = unser(state)
    c, p = prove_on(case, t, b)
    return c, p, ser(t)


# ---- the golden pool (tests/golden/agg_transcript_cases.json): per shape
#   mixed   one instance per position of mixed_positions, instance b proved on state_at(label, pos_b, salt = b)
#   shared  instances proved on ONE state (position 60)
#   for every instance the oracle's prover state; the verifier reaches the same state on an accepted proof
#   corrupted rows of the mixed pool (entry, class) -> (accept, flagged, state_out)
SHAPES = [(2, 4, 4), (3, 4, 4), (6, 2, 3), (16, 16, 16)]
SHARED_POS = 60
SHARED_POOL = {(16, 16, 16): 1}          # instances on the shared state (default 2)
CLASSES = ("wrong_point", "scalar_bit", "V_swapped", "R_off_curve")


def corrupt(case, C: np.ndarray, Q: np.ndarray, kind: str):
    """One row (commitments [k, 64], proof [proof_bytes]) corrupted in place by a field class of agg_cases.corrupted_batch."""
    off = A.field_offsets(case)
    if kind == "wrong_point":
        Q[off["c_r"]:off["c_r"] + 64] = Q[off["c_s"]:off["c_s"] + 64].copy()
    elif kind == "scalar_bit":
        Q[off["n"] + 31] ^= 1
    elif kind == "V_swapped":
        C[[0, 1]] = C[[1, 0]]
    elif kind == "R_off_curve":
        Q[off["R_mid"] + 40] ^= 1
    else:
        raise KeyError(kind)


def shared_state(case) -> bytes:
    return state_at(case["label"], SHARED_POS, salt=99)


def mixed_state(case, b: int) -> bytes:
    pos = mixed_positions(case["label"])
    return state_at(case["label"], pos[b % len(pos)], salt=b)
