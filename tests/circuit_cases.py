"""Seeded generic ArithmeticCircuit instances (circuit.rs) built with the oracle: the reference's own `ac_works` statement
(tests.rs:45-136: x + y = r, x * y = z with dim_nm = 1, dim_no = 2, dim_nv = 2, k = 1, f_l only, LL partition) and random
satisfiable circuits with k > 1, mixed partitions and f_m.

Relation the restated prover is complete for (established by proving and verifying with the oracle, see test_oracle_c.py):
    w = w_l || w_r || w_o,   0 = W_l w + f_l w_V + a_l,   w_l o w_r = W_m w - f_m w_V + a_m,   w_V = v_0 || ... || v_{k-1},
with the f_m form holding for dim_nv = 1 only: for dim_nv > 1, and for f_l and f_m together, the reference's coefficient
helpers (circuit.rs:559-582, 584-599) weight the entries of v inconsistently with mu_vec and its own prover's output does not
verify.  Those shapes are still parity cases -- the verifier must compute the same C0, c and accept bit (0) as the oracle."""
import ctypes as C
import hashlib

import numpy as np

import bppp_oracle as O
import bppp_oracle_c as OC

N = O.N
TYPES = ("LO", "LL", "LR", "NO")


def _sc(tag: bytes, *idx) -> int:
    return O.wide_reduce(hashlib.shake_256(b"bppp-circuit-cases" + tag + b"".join(int(i).to_bytes(4, "little") for i in idx)).digest(64))


def _pow2_at_least(n):
    p = 1
    while p < n:
        p *= 2
    return p


def _b(vals):
    return b"".join(O.sc_to_bytes(v % N) for v in vals)


def ac_works_statement():
    """tests.rs:45-136 with its fixed small witness (x = 3, y = 5, r = 8, z = 15)."""
    x, y, r, z = 3, 5, 8, 15
    W_m = [[0, 0, 1, 0]]
    W_l = [[0, 1, 0, 0], [0, N - 1, 1, 0]]
    return dict(nm=1, no=2, nv=2, k=1, f_l=True, f_m=False, W_m=W_m, W_l=W_l, a_m=[0], a_l=[N - r, N - z],
                part={"LO": [-1, -1], "LL": [0, 1], "LR": [-1, -1], "NO": [-1]},
                w_l=[x], w_r=[y], w_o=[z, r], v=[[x, y]])


def random_statement(tag: bytes, nm, no, nv, k, f_l, f_m, part, density=3):
    """Random witness, random sparse W_m / W_l, a_m / a_l solved from the relation."""
    nl, nw = nv * k, 2 * nm + no
    w_l = [_sc(tag + b"wl", i) for i in range(nm)]
    w_r = [_sc(tag + b"wr", i) for i in range(nm)]
    w_o = [_sc(tag + b"wo", i) for i in range(no)]
    v = [[_sc(tag + b"v", j, i) for i in range(nv)] for j in range(k)]
    w = w_l + w_r + w_o
    wV = [x for row in v for x in row]

    def sparse(rows, t):
        M = [[0] * nw for _ in range(rows)]
        for i in range(rows):
            for c in range(nw):
                h = hashlib.shake_256(tag + t + bytes([i, c])).digest(2)
                if h[0] % density == 0:
                    M[i][c] = [1, N - 1, 2, _sc(tag + t + b"val", i, c)][h[1] % 4]
        return M

    W_m, W_l = sparse(nm, b"Wm"), sparse(nl, b"Wl")
    dot = lambda row: sum(a * b for a, b in zip(row, w)) % N
    a_m = [(w_l[i] * w_r[i] - dot(W_m[i]) + (wV[i] if f_m else 0)) % N for i in range(nm)]
    a_l = [(-dot(W_l[i]) - (wV[i] if f_l else 0)) % N for i in range(nl)]
    return dict(nm=nm, no=no, nv=nv, k=k, f_l=f_l, f_m=f_m, W_m=W_m, W_l=W_l, a_m=a_m, a_l=a_l, part=part, w_l=w_l, w_r=w_r, w_o=w_o, v=v)


STATEMENTS = {
    "ac_works": ac_works_statement,
    # w_o spread over all four partition types, two committed vectors
    "mixed_k2": lambda: random_statement(b"mixed", 4, 4, 3, 2, True, False,
                                         {"LO": [1, -1, -1], "LL": [-1, 2, -1], "LR": [-1, -1, 3], "NO": [-1, 0, -1, -1]}),
    # f_l and f_m together: exercises collect_lambda's tensor terms; the oracle REJECTS its own prover's output here (see above)
    "fl_fm": lambda: random_statement(b"flfm", 4, 2, 2, 2, True, True,
                                      {"LO": [0, -1], "LL": [-1, 1], "LR": [-1, -1], "NO": [-1, -1, -1, -1]}),
    # f_m only with one-element committed vectors: the shape the f_m path is complete for
    "fm_nv1": lambda: random_statement(b"fm1", 3, 2, 1, 3, False, True, {"LO": [0], "LL": [1], "LR": [-1], "NO": [-1, -1, -1]}),
}


def _part(nm, nv, **at):
    """partition tables with w_o index `i` at position `j` of type `typ` for typ=(j, i) or typ=[(j, i), ...]; None everywhere else"""
    p = {"LO": [-1] * nv, "LL": [-1] * nv, "LR": [-1] * nv, "NO": [-1] * nm}
    for typ, where in at.items():
        for j, i in ([where] if isinstance(where, tuple) else where):
            p[typ][j] = i
    return p


def _family(tag, nm, no, nv, k, f_l, f_m, **at):
    fn = lambda: random_statement(b"family-" + tag, nm, no, nv, k, f_l, f_m, _part(nm, nv, **at))
    fn.dims = (nm, no, nv, k)
    return fn


# The shape family: what the statement's shape steers in circuit_core.h / circuit_prove_core.h.  With P = 4 + k points in C0's variable-base
# sum: the lane-per-point form runs on L = the power of two >= P (at least 8) lanes up to L = 64 and the one-lane kernels walk the points in
# chunks of five; NH = the power of two >= nv + 9, NG = the power of two >= nm.  LR entries stay at position nv - 1 (an LR entry in front of it
# leaves the reference's prover incomplete, as f_l + f_m and f_m with nv > 1 do: COMPLETE below).
FAMILY = {
    "k4": _family(b"k4", 2, 2, 2, 4, True, False, LO=(0, 0), LL=(1, 1)),                 # P = 8: L = 8 with no idle lane, chunks 5 + 3
    "k5": _family(b"k5", 2, 1, 1, 5, True, False, LO=(0, 0)),                            # P = 9: L = 16, chunks 5 + 4
    "k11": _family(b"k11", 2, 1, 1, 11, True, False, LL=(0, 0)),                         # P = 15: L = 16, three full chunks
    "k13": _family(b"k13", 3, 0, 1, 13, True, False),                                    # P = 17: L = 32, 5 + 5 + 5 + 2; no w_o at all
    "k60": _family(b"k60", 2, 1, 1, 60, True, False, LO=(0, 0)),                         # P = 64: L = 64, a whole wavefront, no idle lane
    "k61": _family(b"k61", 2, 1, 1, 61, True, False, LR=(0, 0)),                         # P = 65: the one-lane kernels at any size, 13 chunks
    "nv8": _family(b"nv8", 4, 2, 8, 2, True, False, LO=(0, 0), LL=(3, 1)),               # nv + 9 = 17: NH = 32
    "nm5": _family(b"nm5", 5, 2, 2, 1, True, False, NO=(0, 0), LL=(1, 1)),               # NG = 8 with three padding generators
    "nm7": _family(b"nm7", 7, 2, 2, 1, True, False, NO=(6, 0), LO=(1, 1)),               # NG = 8 with one
    "nm8": _family(b"nm8", 8, 2, 2, 1, True, False, NO=(3, 0), LL=(0, 1)),               # NG = nm = 8
    "nm16": _family(b"nm16", 16, 2, 2, 1, True, False, NO=[(0, 0), (15, 1)]),            # NG = nm = NH = 16
    "nof": _family(b"nof", 2, 2, 2, 2, False, False, LO=(0, 0), LR=(1, 1)),              # neither flag: every 2 tau^3 coef_i is zero
    "fm_nv2": _family(b"fm2", 4, 2, 2, 2, False, True, LO=(0, 0), LL=(1, 1)),            # f_m at more than one position (nl = nm)
    "fl_fm_k5": _family(b"flfm5", 5, 1, 1, 5, True, True, LO=(0, 0)),                    # collect_lambda's tensor terms past k = 2 (nl = nm), L = 16
}
STATEMENTS.update(FAMILY)

# Whether the reference's verifier accepts its own prover's output: the C oracle's verdict on the honest proofs of make(name, .), recorded
# here and checked against that verdict by tests/test_circuit_emul.py (test_complete_table_is_the_oracles_verdict).
COMPLETE = {
    "ac_works": True, "mixed_k2": True, "fl_fm": False, "fm_nv1": True,
    "k4": True, "k5": True, "k11": True, "k13": True, "k60": True, "k61": True, "nv8": True, "nm5": True, "nm7": True, "nm8": True,
    "nm16": True, "nof": True, "fm_nv2": False, "fl_fm_k5": False,
}


def c0_lanes(name):
    """L of the lane-per-point form for the statement: the power of two >= 4 + k, at least 8"""
    k = FAMILY[name].dims[3] if name in FAMILY else STATEMENTS[name]()["k"]
    return max(8, _pow2_at_least(4 + k))


# the launch forms the family is there for -> the statements that reach each
LAUNCH_FORMS = {
    "L=8": [n for n in FAMILY if c0_lanes(n) == 8], "L=16": [n for n in FAMILY if c0_lanes(n) == 16],
    "L=32": [n for n in FAMILY if c0_lanes(n) == 32], "L=64": [n for n in FAMILY if c0_lanes(n) == 64],
    "one lane past 64 points": [n for n in FAMILY if c0_lanes(n) > 64],
    "NH=32": ["nv8"], "NG padded": ["nm5", "nm7", "fl_fm_k5"], "NG exact": ["nm8", "nm16"], "no flag": ["nof"],
}


def make(name: str, B: int, label: bytes = b"circuit test"):
    st = STATEMENTS[name]()
    nm, no, nv, k = st["nm"], st["no"], st["nv"], st["k"]
    nl, nw, nh = nv * k, 2 * nm + no, nv + 9
    NG, NH = _pow2_at_least(nm), _pow2_at_least(nh)
    pt = lambda tag, i: OC.point_mul(None, O.sc_to_bytes(_sc(b"gen" + tag, i)))
    g = pt(b"g", 0)
    gv = [pt(b"gv", i) for i in range(nm)]
    hv = [pt(b"hv", i) for i in range(nh)]
    gv_ = [pt(b"gv_", i) for i in range(NG - nm)]
    hv_ = [pt(b"hv_", i) for i in range(NH - nh)]
    parts = {t: np.array(st["part"][t], np.int32) for t in TYPES}
    case = dict(st, g=g, gv=gv, hv=hv, gv_=gv_, hv_=hv_, NG=NG, NH=NH, nl=nl, nw=nw, label=label, parts=parts,
                Wm_bytes=_b(x for row in st["W_m"] for x in row), Wl_bytes=_b(x for row in st["W_l"] for x in row),
                am_bytes=_b(st["a_m"]), al_bytes=_b(st["a_l"]))
    L = OC.lib()
    sz = C.c_size_t
    dims = (sz * 6)(nm, no, k, nl, nv, nw)
    case["dims"] = dims
    coms, proofs, shape = [], [], None
    n_rnd = 64
    used = 18 + nv + nm                                  # draws the prover consumes: r_o 7, r_l 6, r_r 5, l_s nv, n_s nm
    sv_all, rnd_all = [], []
    for b in range(B):
        s_v = [_sc(b"sv", b, j) for j in range(k)]
        rnd = _b(_sc(b"rnd", b, i) for i in range(n_rnd))
        sv_all.append(_b(s_v))
        rnd_all.append(rnd[:32 * used])
        com = C.create_string_buffer(64 * k)
        # room for 16 rounds and 16 final scalars: every round halves the longer of the two vectors, so there are at most
        # log2(max(NG, NH)) of them, and the C oracle ends with at most 8 + 8 scalars (checked again on the shape it reports)
        assert max(NG, NH) <= 1 << 16
        pbuf = C.create_string_buffer(64 * (4 + 2 * 16) + 32 * 16)
        rounds, pl, pn = sz(0), sz(0), sz(0)
        rc = L.bppp_oracle_circuit_prove(g, b"".join(gv), b"".join(hv), b"".join(gv_), sz(len(gv_)), b"".join(hv_), sz(len(hv_)), dims,
                                         int(st["f_l"]), int(st["f_m"]), case["Wm_bytes"], case["Wl_bytes"], case["am_bytes"], case["al_bytes"],
                                         parts["LO"].ctypes.data_as(C.c_void_p), parts["LL"].ctypes.data_as(C.c_void_p),
                                         parts["LR"].ctypes.data_as(C.c_void_p), parts["NO"].ctypes.data_as(C.c_void_p),
                                         label, sz(len(label)), _b(x for row in st["v"] for x in row), _b(s_v), _b(st["w_l"]), _b(st["w_r"]),
                                         _b(st["w_o"]), rnd, sz(n_rnd), com, pbuf, C.byref(rounds), C.byref(pl), C.byref(pn))
        assert rc == 0, rc
        sh = (rounds.value, pl.value, pn.value)
        assert sh[0] <= 16 and sh[1] + sh[2] <= 16, (name, sh)
        shape = shape or sh
        assert sh == shape
        nbytes = 64 * (4 + 2 * sh[0]) + 32 * (sh[1] + sh[2])
        coms.append(com.raw)
        proofs.append(pbuf.raw[:nbytes])
    u8 = lambda blobs, *shape_: np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(B, *shape_).copy()
    case.update(s_v=u8(sv_all, k, 32), rnd=u8(rnd_all, used, 32),
                v_bytes=u8([_b(x for row in st["v"] for x in row)] * B, k, nv, 32), wl_bytes=u8([_b(st["w_l"])] * B, nm, 32),
                wr_bytes=u8([_b(st["w_r"])] * B, nm, 32), wo_bytes=u8([_b(st["w_o"])] * B, no, 32))
    case.update(rounds=shape[0], pl=shape[1], pn=shape[2], proof_bytes=len(proofs[0]),
                commitments=np.frombuffer(b"".join(coms), dtype=np.uint8).reshape(B, k, 64).copy(),
                proofs=np.frombuffer(b"".join(proofs), dtype=np.uint8).reshape(B, -1).copy())
    return case


def oracle_verify(case, commitments: bytes, proof: bytes) -> int:
    L = OC.lib()
    sz = C.c_size_t
    p = case["parts"]
    return L.bppp_oracle_circuit_verify(case["g"], b"".join(case["gv"]), b"".join(case["hv"]), b"".join(case["gv_"]), sz(len(case["gv_"])),
                                        b"".join(case["hv_"]), sz(len(case["hv_"])), case["dims"], int(case["f_l"]), int(case["f_m"]),
                                        case["Wm_bytes"], case["Wl_bytes"], case["am_bytes"], case["al_bytes"],
                                        p["LO"].ctypes.data_as(C.c_void_p), p["LL"].ctypes.data_as(C.c_void_p),
                                        p["LR"].ctypes.data_as(C.c_void_p), p["NO"].ctypes.data_as(C.c_void_p), case["label"],
                                        sz(len(case["label"])), commitments, proof, sz(case["rounds"]), sz(case["pl"]), sz(case["pn"]))
