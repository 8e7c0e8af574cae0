"""The device transcript primitives (bp_pp_amd/csrc/merlin.h, verify_ws.h: app_point and the 203-byte state, kernels.h:
for_each_position_group) at every byte position of the sponge's rate, against the Python oracle (bppp_oracle.Strobe128 / Transcript /
keccak_f1600, pinned to hashlib.sha3_256 and merlin's known answer by test_oracle.py), on the three builds of tests/prims:

  gcc, clang  the host builds: the register sponge `strobe` (shift-or rotate, st_uniform the identity)
  gfx950      marked gpu: `strobe` and the LDS sponge `strobe_lds` (two-alignbit rotate, readfirstlane, scalar switch over the state
              words), each in two launch layouts: uniform (a wavefront's 64 lanes share the start position, the body is called directly)
              and grouped (lanes at different positions inside for_each_position_group(preloaded_position_key(..)))

One launch runs one program of at most 8 steps (prims_core.h: TrStep) over its records.  A record is a 203-byte start state plus message
bytes, four affine points, two u64 and the raw operands.  Everything is compared exactly: the 203 bytes after the program (pos, pos_begin
and the flags byte included), every squeezed byte, the challenge words and the canonical flag.  Start states are real ones
(Transcript(label) plus a context message whose length lands on the position) and synthetic ones (random bytes, all-zero, all-ones, one
set bit in each of the 25 words; any pos in 0 .. 165, pos_begin in 0 .. 166).  Per position a wavefront repeats 2 distinct records, a real
and a synthetic one (4 cost more CPU time than test_prims.py takes, see below; the Keccak-f launches hold 32); the oracle runs once per
distinct record.  What the record set covers is asserted from the oracle's own position trace (coverage()) before any
output is looked at.

Records: raw 3218 distinct, steps 4648, lengths 616, programs 1328 (9810 in all over 97 launches; a uniform wavefront holds each of its
records 32 times).  Measured on the CPU tier (gcc and clang together, libraries built): this module 15 s, of which the oracle 10 s;
test_prims.py takes 16 s on the same machine.  With 4 distinct records per position the module took 28 s, so it runs 2."""
import random
import struct

import numpy as np
import pytest

import bppp_oracle as O
from prims import build as PB

R = 166
IN_W, OUT_W, PROG_W, PROD0 = 152, 180, 25, 52
KECCAK_F, KECCAK_RC, ROTL64, ABSORB_CHUNK, RUN_F, SQUEEZE, META_AD, AD, PRF = range(1, 10)
APPEND_MEM, APPEND_WORDS, APPEND_U64, APP_POINT, GET_CHALLENGE, CHALLENGE_BYTES = range(16, 22)
TRANSCRIPT_KINDS = (APPEND_MEM, APPEND_WORDS, APPEND_U64, APP_POINT, GET_CHALLENGE, CHALLENGE_BYTES)
REGS_ONLY = (META_AD, AD, PRF, APPEND_MEM)
REGS, LDS = 0, 1
UNIFORM, GROUPED = 0, 1
ST_OK, ST_BAD_PARAM, TR_BAD_STATE, TR_BAD_LAYOUT = 0, 2, 4, 5
# prims_core.h: TR_LABELS_ANY, TR_LABELS_POINT, TR_LABELS_CHAL
LABELS = [b"dom-sep", b"l.sz", b"n.sz", b"wnla_challenge", b"circuit_rho", b"reciprocal_challenge", b"a", b"bc", b"def", b"ghijk",
          b"lmnopq", b"wnla_com", b"wnla_x", b"wnla_r", b"reciprocal_commitment", b"commitment_cl", b"commitment_cr", b"commitment_co",
          b"commitment_v", b"commitment_cs", b"circuit_lambda", b"circuit_beta", b"circuit_delta", b"circuit_tau"]
LAB = {s: i for i, s in enumerate(LABELS)}
N_ANY = 11
DISTINCT = 2                                  # distinct records per position; a uniform wavefront repeats them cyclically
FEW = (0, 29, 97, 161, 162, 163, 164, 165)    # the positions of the programs that are about a length, not about the position
ALL = tuple(range(R))
FAMILIES = ("raw", "steps", "lengths", "programs")


# ---------------------------------------------------------------- start states and record contents
def load_state(b: bytes) -> "O.Transcript":
    """The inverse of transcript_cases.ser: an oracle transcript from the 203 bytes."""
    t = object.__new__(O.Transcript)
    s = object.__new__(O.Strobe128)
    s.state = bytearray(b[:200])
    s.pos, s.pos_begin, s.cur_flags = b[200], b[201], b[202]
    t.strobe = s
    return t


def ser(t) -> bytes:
    return bytes(t.strobe.state) + bytes([t.strobe.pos, t.strobe.pos_begin, t.strobe.cur_flags])


def special_states():
    """all-zero, all-ones, and one set bit in each of the 25 words (each rho amount in isolation; the bit moves with the word)"""
    out = [bytes(200), b"\xFF" * 200]
    for w in range(25):
        out.append(struct.pack("<25Q", *[(1 << ((7 * w + 3) % 64)) if i == w else 0 for i in range(25)]))
    return out


_POINTS = None


def points():
    """oracle points: [identity, y odd, y even, ...]"""
    global _POINTS
    if _POINTS is None:
        pts = [O.pt_mul(O.G, k) for k in (1, 2, 3, 5, 7, 11)]
        odd = [p for p in pts if p[1] & 1]
        even = [p for p in pts if not p[1] & 1]
        assert odd and even
        _POINTS = [None, odd[0], even[0]] + [p for p in pts if p not in (odd[0], even[0])]
    return _POINTS


def limbs26(x):
    return [(x >> (26 * i)) & ((1 << 26) - 1) for i in range(9)] + [x >> 234]


class Content:
    """what a record holds beside its state"""

    def __init__(self, rg, c):      # c: a number that runs over the records, so that every variant below meets every position class
        self.msg = bytes(rg.randrange(1, 256) for _ in range(256))       # no zero byte: a dropped byte always shows
        P = points()
        self.pts = [P[(c + k) % 3] if k < 3 else P[3 + c % (len(P) - 3)] for k in range(4)]      # slot 0: identity, odd, even by c
        self.u64 = [rg.getrandbits(64), (32 >> (c % 4)) if c % 2 else rg.getrandbits(64)]
        self.rot = [rg.getrandbits(64), 1, 1 << 63, (1 << 64) - 1][c % 4]
        self.word = int.from_bytes(bytes(rg.randrange(1, 256) for _ in range(4)), "little")

    def words(self):
        w = list(struct.unpack("<64I", self.msg))
        for p in self.pts:
            w += [0] * 20 if p is None else limbs26(p[0]) + limbs26(p[1])
        for x in self.u64 + [self.rot]:
            w += [x & 0xFFFFFFFF, x >> 32]
        w += [self.word, 0]
        assert len(w) == IN_W
        return w


_STATES = None


def start_states():
    """[pos][c] -> 203 bytes: c = 0 real (Transcript(label) + a context message that lands on pos, at odd positions a rate longer),
    c = 1 synthetic: at even positions random bytes with pos_begin = 166 - pos, at odd ones a special state with pos_begin at the
    ends of its range first, then spread over it"""
    global _STATES
    if _STATES is None:
        rg = random.Random(20250)
        base = O.Transcript(b"bp-pp-amd/prims")
        off = (base.strobe.pos + 2 + 3 + 4 + 2) % R          # position after append_message(b"ctx", b"")
        sp = special_states()
        _STATES = []
        for p in range(R):
            t = base.clone()
            t.append_message(b"ctx", bytes(rg.randrange(256) for _ in range((p - off) % R + R * (p % 2))))
            assert t.strobe.pos == p
            if p % 2 == 0:
                syn = bytes(rg.randrange(256) for _ in range(200)) + bytes([p, R - p, rg.choice((2, 7, 18))])
            else:
                syn = sp[(p // 2) % len(sp)] + bytes([p, (0, 1, R - 1, R)[p // 2] if p < 8 else (7 * p) % (R + 1), 2])
            _STATES.append([ser(t), syn])
    return _STATES


_CONTENTS = None


def contents():
    global _CONTENTS
    if _CONTENTS is None:
        rg = random.Random(77)
        _CONTENTS = [[Content(rg, p + c) for c in range(DISTINCT)] for p in range(R)]
    return _CONTENTS


# ---------------------------------------------------------------- programs
class Launch:
    """one program over the DISTINCT records of each of its positions; states[pi][c], recs[pi][c]"""

    def __init__(self, family, name, steps, positions=ALL, states=None):
        assert 0 < len(steps) <= 8
        self.family, self.name, self.steps, self.positions = family, name, steps, tuple(positions)
        S, C = start_states(), contents()
        self.states = states if states is not None else [[S[p][c] for c in range(DISTINCT)] for p in self.positions]
        self.contents = [[C[p][c % DISTINCT] for c in range(len(self.states[i]))] for i, p in enumerate(self.positions)]
        self.lds = all(k not in REGS_ONLY for k, _, _ in steps)

    def prog(self):
        w = [len(self.steps)]
        for k, lab, par in self.steps:
            w += [k, lab, par]
        return np.array(w + [0] * (PROG_W - len(w)), np.uint32)


def T(kind, label, par=0):
    return (kind, LAB[label], par)


_LAUNCHES = None


def launches():
    global _LAUNCHES
    if _LAUNCHES is not None:
        return _LAUNCHES
    L = []
    # ---- raw steps
    sp = special_states()
    rg = random.Random(5)
    for p in (0, 165):       # Keccak-f alone: every special state and random ones, beside two positions it must not look at
        sts = [[s + bytes([p, (p + 1) % (R + 1), 2]) for s in sp + [bytes(rg.randrange(256) for _ in range(200)) for _ in range(5)]]]
        L.append(Launch("raw", f"keccak_f pos {p}", [(KECCAK_F, 0, 0)], (p,), sts))
    for q in range(3):
        L.append(Launch("raw", f"keccak_rc {8 * q}..", [(KECCAK_RC, 0, 8 * q + i) for i in range(8)], (0,)))
    for q in range(8):
        L.append(Launch("raw", f"rotl64 {8 * q}..", [(ROTL64, 0, r) for r in range(max(8 * q, 1), 8 * q + 8)], (0, 9)))
    for nb in (1, 2, 3, 4):
        L.append(Launch("raw", f"absorb_chunk {nb}", [(ABSORB_CHUNK, 0, nb)]))
    L.append(Launch("raw", "run_f", [(RUN_F, 0, 0)]))
    L.append(Launch("raw", "squeeze 5", [(SQUEEZE, 0, 5)]))
    for n in (0, 1, 32, 167, 200):
        L.append(Launch("raw", f"squeeze {n}", [(SQUEEZE, 0, n)], FEW))
    L.append(Launch("raw", "meta_ad 3", [(META_AD, 0, 3)]))
    L.append(Launch("raw", "ad 5", [(AD, 0, 5)]))
    L.append(Launch("raw", "prf 9", [(PRF, 0, 9)]))
    L.append(Launch("raw", "meta_ad, more, ad = append_message", [(META_AD, 0, 3), (META_AD, 0, 4 | 1 << 16), (AD, 0, 256)], FEW))
    L.append(Launch("raw", "ad 0, ad more 200, prf 40", [(AD, 0, 0), (AD, 0, 200 | 1 << 16), (PRF, 0, 40)], FEW))
    L.append(Launch("raw", "chunks, run_f, keccak_f, squeeze",
                    [(ABSORB_CHUNK, 0, 4), (ABSORB_CHUNK, 0, 3), (RUN_F, 0, 0), (ABSORB_CHUNK, 0, 2), (KECCAK_F, 0, 0), (SQUEEZE, 0, 7)], FEW))
    # ---- every transcript step kind, and every label of the ANY list, as the first step from each position
    L.append(Launch("steps", "append_mem dom-sep 37", [T(APPEND_MEM, b"dom-sep", 37)]))
    L.append(Launch("steps", "append_words ghijk 35", [T(APPEND_WORDS, b"ghijk", 35)]))
    L.append(Launch("steps", "append_u64 l.sz", [T(APPEND_U64, b"l.sz", 0)]))
    L.append(Launch("steps", "app_point wnla_com", [T(APP_POINT, b"wnla_com", 0)]))
    L.append(Launch("steps", "get_challenge wnla_challenge", [T(GET_CHALLENGE, b"wnla_challenge")]))
    L.append(Launch("steps", "challenge_bytes reciprocal_challenge 64", [T(CHALLENGE_BYTES, b"reciprocal_challenge", 64)]))
    L.append(Launch("steps", "append_u64 n.sz", [T(APPEND_U64, b"n.sz", 1)]))
    L.append(Launch("steps", "get_challenge circuit_rho", [T(GET_CHALLENGE, b"circuit_rho")]))
    L.append(Launch("steps", "append_words a 34", [T(APPEND_WORDS, b"a", 34)]))
    L.append(Launch("steps", "app_point bc", [T(APP_POINT, b"bc", 1)]))
    L.append(Launch("steps", "challenge_bytes def 33", [T(CHALLENGE_BYTES, b"def", 33)]))
    L.append(Launch("steps", "append_mem lmnopq 6", [T(APPEND_MEM, b"lmnopq", 6)]))
    L.append(Launch("steps", "append_words lmnopq 36", [T(APPEND_WORDS, b"lmnopq", 36)]))      # the LDS sponge has no append from memory
    L.append(Launch("steps", "append_u64 dom-sep", [T(APPEND_U64, b"dom-sep", 0)]))
    # ---- lengths
    for n in range(37):
        L.append(Launch("lengths", f"append_words def {n}", [T(APPEND_WORDS, b"def", n)], FEW if n % 4 == 1 else FEW[3:]))
    for n in (0, 1, 165, 166, 167, 200):
        L.append(Launch("lengths", f"append_mem bc {n}", [T(APPEND_MEM, b"bc", n)], FEW))
    for n in (0, 1, 31, 32, 167, 200):
        L.append(Launch("lengths", f"challenge_bytes a {n}", [T(CHALLENGE_BYTES, b"a", n)], FEW))
    # ---- the protocols' longest transcript sequences, from each position
    L.append(Launch("programs", "wnla_verify_round",
                    [T(APP_POINT, b"wnla_com", 0), T(APP_POINT, b"wnla_x", 1), T(APP_POINT, b"wnla_r", 2), T(APPEND_U64, b"l.sz", 0),
                     T(APPEND_U64, b"n.sz", 1), T(GET_CHALLENGE, b"wnla_challenge")]))
    L.append(Launch("programs", "verify_phase1_on, first 8",
                    [T(APP_POINT, b"reciprocal_commitment", 0), T(GET_CHALLENGE, b"reciprocal_challenge"), T(APP_POINT, b"commitment_cl", 1),
                     T(APP_POINT, b"commitment_cr", 2), T(APP_POINT, b"commitment_co", 3), T(APP_POINT, b"commitment_v", 0),
                     T(GET_CHALLENGE, b"circuit_rho"), T(GET_CHALLENGE, b"circuit_lambda")]))
    L.append(Launch("programs", "circuit_phase1, first 8",
                    [T(APP_POINT, b"commitment_cl", 0), T(APP_POINT, b"commitment_cr", 1), T(APP_POINT, b"commitment_co", 2),
                     T(APP_POINT, b"commitment_v", 3), T(GET_CHALLENGE, b"circuit_rho"), T(GET_CHALLENGE, b"circuit_lambda"),
                     T(GET_CHALLENGE, b"circuit_beta"), T(GET_CHALLENGE, b"circuit_delta")]))
    L.append(Launch("programs", "circuit_phase1, the rest",
                    [T(GET_CHALLENGE, b"circuit_beta"), T(GET_CHALLENGE, b"circuit_delta"), T(APP_POINT, b"commitment_cs", 1),
                     T(GET_CHALLENGE, b"circuit_tau")]))
    _LAUNCHES = L
    return L


# ---------------------------------------------------------------- the reference model
def pack_bytes(b):
    b = bytes(b) + bytes(-len(b) % 4)
    return list(struct.unpack(f"<{len(b) // 4}I", b))


def model(steps, state, c):
    """The oracle over one record: (expected output row, trace).  trace: ("chunk", step, what, start, nb, bytes) for every chunk of 2 to
    4 bytes the device code absorbs (transcript steps, raw chunk steps, the operation headers of the raw STROBE steps), start = the
    oracle's position there (a header's first byte is given as 0: only its flags byte can be carried); ("prf_end", step, e) with e the
    position where a challenge's PRF header ends (0: exactly at the rate); ("run_f", step, pos) for a permutation run before the rate is
    full; ("squeeze", step, start, n)."""
    t = load_state(state)
    s = t.strobe
    prod, trace = [], []
    for si, (kind, lab, par) in enumerate(steps):
        label = LABELS[lab]
        pos0 = s.pos
        if kind in TRANSCRIPT_KINDS:
            LL = len(label)
            nbytes = {APPEND_U64: 8, APP_POINT: 33, GET_CHALLENGE: 32}.get(kind, par)
            trace.append(("chunk", si, "header", pos0, 2, bytes([0, 18])))
            for k in range(0, LL, 4):
                trace.append(("chunk", si, "label", (pos0 + 2 + k) % R, min(4, LL - k), label[k:k + 4]))
            trace.append(("chunk", si, "length", (pos0 + 2 + LL) % R, 4, struct.pack("<I", nbytes)))
            trace.append(("chunk", si, "header", (pos0 + 6 + LL) % R, 2, bytes([0, 7 if kind in (GET_CHALLENGE, CHALLENGE_BYTES) else 2])))
        if kind in (META_AD, AD, PRF) and not (kind != PRF and par >> 16):
            trace.append(("chunk", si, "header", pos0, 2, bytes([0, {META_AD: 18, AD: 2, PRF: 7}[kind]])))
            if kind == PRF and (pos0 + 2) % R:
                trace.append(("run_f", si, (pos0 + 2) % R))
        if kind == KECCAK_F:
            O.keccak_f1600_bytes(s.state)
        elif kind == KECCAK_RC:
            prod += [O._RC[par] & 0xFFFFFFFF, O._RC[par] >> 32]
        elif kind == ROTL64:
            v = ((c.rot << par) | (c.rot >> (64 - par))) & ((1 << 64) - 1)
            prod += [v & 0xFFFFFFFF, v >> 32]
        elif kind == ABSORB_CHUNK:
            trace.append(("chunk", si, "raw", pos0, par, c.word.to_bytes(4, "little")[:par]))
            s._absorb(c.word.to_bytes(4, "little")[:par])
        elif kind == RUN_F:
            trace.append(("run_f", si, pos0))
            s._run_f()
        elif kind == SQUEEZE:
            trace.append(("squeeze", si, pos0, par))
            prod += pack_bytes(s._squeeze(par))
        elif kind in (META_AD, AD):
            n, more = par & 0xFFFF, par >> 16
            if more:
                s._absorb(c.msg[:n])        # a continued operation begins nothing, whatever the flags were
            elif kind == META_AD:
                s.meta_ad(c.msg[:n], False)
            else:
                s.ad(c.msg[:n], False)
        elif kind == PRF:
            prod += pack_bytes(s.prf(par, False))
        elif kind in (APPEND_MEM, APPEND_WORDS, APPEND_U64, APP_POINT):
            if kind == APPEND_U64:
                m = struct.pack("<Q", c.u64[par])
                t.append_u64(label, c.u64[par])
            elif kind == APP_POINT:
                m = O.pt_to_bytes(c.pts[par])
                O.app_point(label, c.pts[par], t)
            else:
                m = c.msg[:par]
                t.append_message(label, m)
            for k in range(0, len(m), 4):
                trace.append(("chunk", si, "message", (pos0 + 8 + len(label) + k) % R, min(4, len(m) - k), m[k:k + 4]))
        else:
            n = 32 if kind == GET_CHALLENGE else par
            trace.append(("prf_end", si, (pos0 + 8 + len(label)) % R))
            if (pos0 + 8 + len(label)) % R:
                trace.append(("run_f", si, (pos0 + 8 + len(label)) % R))
            b = t.challenge_bytes(label, n)
            trace.append(("squeeze", si, 0, n))
            if kind == GET_CHALLENGE:
                v = int.from_bytes(b, "big")
                prod += [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [1 if v < O.N else 0]
            else:
                prod += pack_bytes(b)
    row = pack_bytes(ser(t)) + [ST_OK] + prod
    return np.array(row + [0] * (OUT_W - len(row)), np.uint32), trace


def straddles(trace):
    """the chunks of a record that straddle the rate (strobe_absorb_chunk's take < nb)"""
    return [e for e in trace if e[0] == "chunk" and e[3] + e[4] > R]


def carries(trace):
    """the straddling chunks whose bytes past the rate are not all zero (the length word of a short message and an all-zero message
    carry zeros: dropping those changes nothing)"""
    return [e for e in straddles(trace) if any(e[5][R - e[3]:])]


def crosses_word(trace):
    """what st_xor_bytes writes into the next 64-bit state word from a shift above 32 (its v1): chunks, the straddling ones by their part
    below the rate, and the two bytes strobe_run_f writes at a position that is 7 mod 8"""
    return [e for e in trace if (e[0] == "chunk" and (e[3] & 7) >= 5 and (e[3] & 7) + min(e[4], R - e[3]) > 8) or
            (e[0] == "run_f" and (e[2] & 7) == 7)]


_REF = {}


def reference(li):
    """expected rows [pi][c] and traces of launch number li, computed once"""
    if li not in _REF:
        Ln = launches()[li]
        rows, traces = [], []
        for sts, cs in zip(Ln.states, Ln.contents):
            mt = [model(Ln.steps, s, c) for s, c in zip(sts, cs)]
            rows.append([m[0] for m in mt])
            traces.append([m[1] for m in mt])
        _REF[li] = (rows, traces)
    return _REF[li]


# ---------------------------------------------------------------- what the record set covers
_COVERED = []


def coverage():
    """Asserted over the record set and the oracle's position trace alone, before any output is looked at."""
    if _COVERED:
        return
    Ls = launches()
    for form in (REGS, LDS):
        kinds = [k for k in TRANSCRIPT_KINDS if form == REGS or k not in REGS_ONLY]
        first = {k: set() for k in kinds}
        for Ln in Ls:
            if (form == REGS or Ln.lds) and Ln.steps[0][0] in first:
                first[Ln.steps[0][0]] |= set(Ln.positions)
        assert all(first[k] == set(ALL) for k in kinds), f"a step kind misses a start position on form {form}"
        for cls in range(4):          # label length mod 4
            at = set()
            for Ln in Ls:
                k, lab, _ = Ln.steps[0]
                if (form == REGS or Ln.lds) and k in TRANSCRIPT_KINDS and len(LABELS[lab]) % 4 == cls:
                    at |= set(Ln.positions)
            assert at == set(ALL), f"label length class {cls} misses a position on form {form}"
        for lab in range(N_ANY):
            at = set()
            for Ln in Ls:
                if (form == REGS or Ln.lds) and Ln.steps[0][0] in TRANSCRIPT_KINDS and Ln.steps[0][1] == lab:
                    at |= set(Ln.positions)
            assert at == set(ALL), f"label {LABELS[lab]} misses a position on form {form}"
        strad, prf_end, squeeze_cross = set(), set(), False
        for li, Ln in enumerate(Ls):
            if form == LDS and not Ln.lds:
                continue
            for tr_row in reference(li)[1]:
                for tr in tr_row:
                    for e in straddles(tr):
                        strad.add((e[2], e[4], e[3]))
                    for e in tr:
                        if e[0] == "prf_end":
                            prf_end.add(e[2])
                        if e[0] == "squeeze" and e[3] >= 167 and e[2] + e[3] > R:
                            squeeze_cross = True
        for nb, starts in ((2, (165,)), (3, (164, 165)), (4, (163, 164, 165))):
            for what in ("header", "label", "length", "message", "raw"):
                if (what == "header" and nb != 2) or (what == "length" and nb != 4):
                    continue          # a header chunk is 2 bytes, the length word 4
                for st in starts:
                    assert (what, nb, st) in strad, f"no {what} chunk of {nb} bytes straddles from {st} on form {form}"
        assert 0 in prf_end and 165 in prf_end, "no PRF header ends exactly at the rate / one byte before it"
        assert squeeze_cross, "no squeeze of 167 bytes or more"
    wl = {par for Ln in Ls for k, _, par in Ln.steps if k == APPEND_WORDS}
    assert wl >= set(range(37))
    ml = {par for Ln in Ls for k, _, par in Ln.steps if k == APPEND_MEM}
    assert ml >= {0, 1, 165, 166, 167, 200}
    assert {par for Ln in Ls for k, _, par in Ln.steps if k == ROTL64} == set(range(1, 64))
    assert {par for Ln in Ls for k, _, par in Ln.steps if k == KECCAK_RC} == set(range(24))
    assert {par for Ln in Ls for k, _, par in Ln.steps if k == ABSORB_CHUNK} == {1, 2, 3, 4}
    S = start_states()
    assert {S[p][1][201] for p in ALL} >= {0, 1, 165, 166}
    slot0 = {(None if c.pts[0] is None else c.pts[0][1] & 1) for row in contents() for c in row}
    assert slot0 == {None, 0, 1}, "app_point needs the identity, an odd and an even y"
    _COVERED.append(True)


def test_record_set_covers_every_position_and_edge():
    coverage()


# ---------------------------------------------------------------- running
def arrange(Ln, layout, alternate=False):
    """The launch's records in launch order, as (pi, c) pairs.  Uniform: a wavefront per position, its 64 lanes repeating the
    position's distinct records.  Grouped: record c of every position, then record c + 1, ...: consecutive lanes hold consecutive
    positions, so that a lane is alone or nearly alone in its group.  alternate: two positions by turns within each wavefront."""
    npos = len(Ln.positions)
    if alternate:
        half = npos // 2
        return [((w if lane % 2 == 0 else w + half), (lane // 2) % len(Ln.states[w])) for w in range(half) for lane in range(64)]
    if layout == UNIFORM:
        return [(pi, lane % len(Ln.states[pi])) for pi in range(npos) for lane in range(64)]
    return [(pi, c) for c in range(max(len(s) for s in Ln.states)) for pi in range(npos) if c < len(Ln.states[pi])]


def run_launch(lib, Ln, form, layout, order):
    """runs the records `order` of a launch; returns rows [pi][c] after checking that every copy of a record gave the same words"""
    words = [[np.array(c.words(), np.uint32) for c in cs] for cs in Ln.contents]
    states = np.frombuffer(b"".join(Ln.states[pi][c] for pi, c in order), np.uint8).copy()
    recs = np.ascontiguousarray(np.stack([words[pi][c] for pi, c in order]))
    out = np.zeros((len(order), OUT_W), np.uint32)
    prog = Ln.prog()
    rc = lib.run_transcript(prog.ctypes.data, form, layout, states.ctypes.data, recs.ctypes.data, out.ctypes.data, len(order))
    assert rc == 0, f"{Ln.name}: run returned {rc}"
    rows = [[None] * len(s) for s in Ln.states]
    for i, (pi, c) in enumerate(order):
        if rows[pi][c] is None:
            rows[pi][c] = out[i]
        else:
            assert (rows[pi][c] == out[i]).all(), f"{Ln.name}: copies of record (pos {Ln.positions[pi]}, {c}) differ (lane {i % 64})"
    return rows


_LIB, _OUT = {}, {}


def lib_of(backend):
    if backend not in _LIB:
        why = PB.unavailable(backend)
        if why:
            pytest.skip(f"{backend} backend skipped: {why}")
        L = PB.load(backend)
        assert [L.prims_transcript_words(i) for i in range(3)] == [IN_W, OUT_W, PROG_W]
        _LIB[backend] = L
    return _LIB[backend]


def outputs(backend, form=REGS, layout=UNIFORM):
    """{launch number: rows [pi][c]} of every launch the form can run"""
    key = (backend, form, layout)
    if key not in _OUT:
        lib = lib_of(backend)
        coverage()
        _OUT[key] = {li: run_launch(lib, Ln, form, layout, arrange(Ln, layout)) for li, Ln in enumerate(launches())
                     if form == REGS or Ln.lds}
    return _OUT[key]


def compare(out, family, what):
    bad, n = [], 0
    for li, Ln in enumerate(launches()):
        if Ln.family != family or li not in out:
            continue
        exp = reference(li)[0]
        for pi, p in enumerate(Ln.positions):
            for c, e in enumerate(exp[pi]):
                n += 1
                got = out[li][pi][c]
                if not (got == e).all():
                    w = int(np.nonzero(got != e)[0][0])
                    bad.append(f"{Ln.name}, pos {p}, record {c}: word {w} is {int(got[w]):#x}, expected {int(e[w]):#x}")
    assert n > 0
    assert not bad, f"{len(bad)} of {n} {family} records wrong on {what}:\n" + "\n".join(bad[:20])


BACKEND_PARAMS = ["gcc", "clang", pytest.param("gfx950", marks=pytest.mark.gpu)]


@pytest.fixture(scope="module", params=BACKEND_PARAMS)
def backend(request):
    return request.param


@pytest.mark.parametrize("family", FAMILIES)
def test_transcript_primitives(backend, family):
    """The register sponge on every build (the device in the uniform layout) against the oracle, all bits."""
    compare(outputs(backend), family, backend)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_lds_sponge(family):
    """strobe_lds, loaded with strobe_lds_load and stored through ws_st_transcript's layout, against the oracle and the register sponge."""
    out = outputs("gfx950", LDS, UNIFORM)
    compare(out, family, "gfx950 strobe_lds")
    regs = outputs("gfx950")
    for li, rows in out.items():
        if launches()[li].family == family:
            assert all((a == b).all() for ra, rb in zip(rows, regs[li]) for a, b in zip(ra, rb)), launches()[li].name


@pytest.mark.gpu
@pytest.mark.parametrize("form", (REGS, LDS), ids=("strobe", "strobe_lds"))
def test_grouped_layout(form):
    """Every launch again with consecutive lanes at consecutive positions, inside for_each_position_group(preloaded_position_key):
    the oracle's bits, which are the uniform layout's."""
    out = outputs("gfx950", form, GROUPED)
    for family in FAMILIES:
        compare(out, family, f"gfx950 form {form}, grouped")
    uni = outputs("gfx950", form, UNIFORM)
    for li, rows in out.items():
        assert all((a == b).all() for ra, rb in zip(rows, uni[li]) for a, b in zip(ra, rb)), launches()[li].name


@pytest.mark.gpu
@pytest.mark.parametrize("form", (REGS, LDS), ids=("strobe", "strobe_lds"))
def test_two_alternating_positions_per_wavefront(form):
    """Two groups of 32 lanes by turns in every wavefront, through a program with permutations in the middle."""
    lib = lib_of("gfx950")
    coverage()
    for li, Ln in enumerate(launches()):
        if Ln.family != "programs":
            continue
        order = arrange(Ln, GROUPED, alternate=True)
        assert all(len({Ln.positions[pi] for pi, _ in order[w:w + 64]}) == 2 for w in range(0, len(order), 64))
        rows = run_launch(lib, Ln, form, GROUPED, order)
        exp = reference(li)[0]
        for pi, p in enumerate(Ln.positions):
            for c in range(DISTINCT):
                assert (rows[pi][c] == exp[pi][c]).all(), f"{Ln.name}, pos {p}, record {c}"


def bad_state_launch(p):
    """a wavefront at position p whose first lane holds a state strobe_from_bytes refuses with the same raw byte 200 (pos_begin past
    the rate), and a second wavefront whose first lane's byte 200 itself is past the rate"""
    Ln = next(x for x in launches() if x.name == "wnla_verify_round")
    pi = Ln.positions.index(p)
    states, order = [], []
    for bad in (lambda s: s[:201] + bytes([R + 1]) + s[202:], lambda s: s[:200] + bytes([R]) + s[201:]):
        for lane in range(64):
            c = lane % DISTINCT
            states.append(bad(Ln.states[pi][c]) if lane == 0 else Ln.states[pi][c])
            order.append((pi, c))
    return Ln, states, order


def run_raw(lib, Ln, form, layout, states, order):
    words = [[np.array(c.words(), np.uint32) for c in cs] for cs in Ln.contents]
    st = np.frombuffer(b"".join(states), np.uint8).copy()
    recs = np.ascontiguousarray(np.stack([words[pi][c] for pi, c in order]))
    out = np.zeros((len(order), OUT_W), np.uint32)
    prog = Ln.prog()
    rc = lib.run_transcript(prog.ctypes.data, form, layout, st.ctypes.data, recs.ctypes.data, out.ctypes.data, len(order))
    assert rc == 0
    return out


def check_bad_state(lib, form, layout):
    for p in (0, 77, 165):
        Ln, states, order = bad_state_launch(p)
        out = run_raw(lib, Ln, form, layout, states, order)
        exp = reference(launches().index(Ln))[0]
        for i, (pi, c) in enumerate(order):
            if i % 64 == 0:
                assert int(out[i, 51]) == TR_BAD_STATE and not np.delete(out[i], 51).any(), f"pos {p}, lane {i}: not flagged"
            else:
                assert (out[i] == exp[pi][c]).all(), f"pos {p}: lane {i}, beside a refused state, is disturbed"


def test_refused_state_is_flagged_and_not_evaluated(backend):
    """A state strobe_from_bytes refuses is answered with a status and nothing else; on the device (uniform layout) its wavefront
    goes on undisturbed."""
    check_bad_state(lib_of(backend), REGS, UNIFORM)


@pytest.mark.gpu
@pytest.mark.parametrize("form", (REGS, LDS), ids=("strobe", "strobe_lds"))
def test_refused_state_does_not_disturb_its_group(form):
    """Grouped layout: the refused state sits in the wavefront's first lane, which leads the first group, and shares its raw byte 200
    with its 63 neighbours: it gets a key of its own (preloaded_position_key), is flagged, and the neighbours' results stand."""
    check_bad_state(lib_of("gfx950"), form, GROUPED)


def test_same_bits_everywhere(backend):
    """gcc, clang and gfx950 give identical output words for every record."""
    out = outputs(backend)
    others = [b for b in ("gcc", "clang") if b != backend and PB.unavailable(b) is None]
    if not others:
        pytest.skip("no second build to compare with")
    for other in others:
        oo = outputs(other)
        for li, rows in out.items():
            assert all((a == b).all() for ra, rb in zip(rows, oo[li]) for a, b in zip(ra, rb)), f"{backend} vs {other}: {launches()[li].name}"


def test_dispatcher_bounds_every_count(backend):
    """A program past a bound is answered with ST_BAD_PARAM and no evaluation; on the device a uniform launch whose wavefront mixes
    positions is answered with TR_BAD_LAYOUT instead of being run outside the functions' precondition."""
    lib = lib_of(backend)
    Ln = next(x for x in launches() if x.name == "wnla_verify_round")
    bad = [[(SQUEEZE, 0, 201)], [(KECCAK_RC, 0, 24)], [(ROTL64, 0, 0)], [(ROTL64, 0, 64)], [(ABSORB_CHUNK, 0, 5)], [(ABSORB_CHUNK, 0, 0)],
           [(APPEND_MEM, 0, 201)], [(APPEND_WORDS, 0, 37)], [(APPEND_U64, 0, 2)], [(APP_POINT, 0, 4)], [(CHALLENGE_BYTES, 0, 201)],
           [(GET_CHALLENGE, len(LABELS), 0)], [(APPEND_U64, LAB[b"wnla_com"], 0)], [(APP_POINT, LAB[b"circuit_tau"], 0)],
           [(META_AD, 0, 257)], [(AD, 0, 2 << 16)], [(PRF, 0, 201)], [(0, 0, 0)], [(KECCAK_F, 1, 0)], [(15, 0, 0)],
           [(CHALLENGE_BYTES, 0, 200)] * 3, [(KECCAK_F, 0, 0)] * 9]
    order = [(0, c) for c in range(DISTINCT)]
    for steps in bad:
        w = [len(steps)] + [x for s in steps[:8] for x in s]
        prog = np.array(w + [0] * (PROG_W - len(w)), np.uint32)
        st = np.frombuffer(b"".join(Ln.states[0][c] for _, c in order), np.uint8).copy()
        recs = np.ascontiguousarray(np.stack([np.array(Ln.contents[0][c].words(), np.uint32) for _, c in order]))
        out = np.zeros((len(order), OUT_W), np.uint32)
        assert lib.run_transcript(prog.ctypes.data, REGS, UNIFORM, st.ctypes.data, recs.ctypes.data, out.ctypes.data, len(order)) == 0
        assert out[:, 51].tolist() == [ST_BAD_PARAM] * len(order) and not np.delete(out, 51, axis=1).any(), steps
    if backend == "gfx950":
        order = [(lane % 2, 0) for lane in range(64)]
        out = run_raw(lib, Ln, REGS, UNIFORM, [Ln.states[pi][c] for pi, c in order], order)
        assert out[:, 51].tolist() == [TR_BAD_LAYOUT] * 64 and not np.delete(out, 51, axis=1).any()
