"""The aggregated reciprocal range proof's device stages on their RESULTS, not on verdicts: phase 1 and the C0 stage of the verifier
(agg_core.h, k_agg.hip) and the prover's witness, r1, msm and r2 stages (agg_prove_core.h, k_aggprove.hip), every buffer they write against the Python oracle,
on the three builds of tests/prims:

  gcc, clang  the host builds: the single-thread form (agg_phase1_head / run / tail with the runs summed on the host, fb_sum_serial over
              the form's lane count, agg_c0_tables / var / finish, agg_prove_stage_r2)
  gfx950      marked gpu: the product's own kernels -- tests/prims/agg_device.hip includes bp_pp_amd/csrc/k_agg.hip and k_aggprove.hip as
              they are and launches them with the grids of agg_verify_device_impl / agg_prove_part

The verifier rejects every row whose V_i + R_i meets an exception of the group law and every row with two equal points in one chunk of
C0's variable-base sum, whatever the kernels compute there: an identity among the k sums that zeroed the shared product of the Z, a
chunk total dropped by agg_c0_var or a wrong power at a value boundary of a lane group's run would leave every verdict right.  Here a
batch of 71 instances per shape -- honest rows between the special ones, special rows as neighbours, the last row special, a second
wavefront with a ragged end in the one-lane grid and in the G = 8 grid (568 threads) -- is compared per row with the oracle's trace
(agg_cases.verify stopped once C0 is recorded):

  bit for bit   wn_rho, wn_mu, all NH entries of wn_c, sc0 (ps_tau | pn_tau | tau^-1, -delta, tau, -tau^2 | 2 tau^3 lambda^(nv i), the last
                k from ArithmeticCircuit.linear_comb_coef), inv = (e + j)^-1, pts (c_s, c_o, c_l, c_r, then V_i + R_i by the oracle's group
                law, (0, 0) for the identity), status, wn_commit = C0
  as points     pfix = ps_tau g + <g_vec, pn_tau>, acc = the sum of the 4 + k terms

for phase 1 on 1, 2, 4 and 8 lanes, the three fixed-base kernels and both forms of the variable-base sum, each against the oracle; a
malformed row has no trace: its status bit is asserted, and its neighbours equal their own expectations.  Stage r2 runs on crafted rpb
(projective R_i = r G with a random Z) and commitments, k = 3 and 7: cp_vpts and proof_R equal the oracle's affine bytes.

The prover's other stages run on the device build too: k_aprove_witness at the edges of the range, k_aprove_stage_r1 on the witness
kernel's output (big-integer reciprocals, the transcript state behind e), k_aprove_msm with ct = 0 and 1 (tests below).  The verifier's
tstate is compared with the oracle's transcript, rebuilt from the oracle's own call sequence and checked on its challenges.

Which chunks of the variable-base sum take straus_affine<M>'s fallback is asserted per row: the mask recomputed beside the sum
(straus_affine_fast) equals the walk restated on the oracle's group law (expected_fell).  Equal points alone do not force it; FELL
names the classes that take it.

Measured: the CPU tier (gcc and clang together, 79 tests, libraries built) 32 s for this module, its slowest test 3.6 s (the first test
of a shape computes the oracle's expectations for its batch, which every build then shares); on an MI355X the module's 38 gfx950 tests take 10.4 s, the slowest 3.0 s (test_same_bytes_on_every_build, which also
runs both host builds), the slowest that only runs kernels 1.9 s; witness, r1 and msm tests 0.3 s or less each.

One-line mutants, applied one at a time outside the tree, on gfx950 on an MI355X (the module's 38 tests; the untouched units' objects
shared, agg_device.hip recompiled) -- and tests/test_gpu_agg.py + tests/test_gpu_agg_prove.py (52 tests) on the product library
relinked with the mutated k_agg.hip / k_aggprove.hip:
  (a) agg_phase1_head without fe_cmov(z, fe_is_zero(s.Z), one_fe) before the product      28 of 38 fail; the two modules: 52 pass
  (b) agg_prove_stage_r2's to_affine without fe_cmov(a.x, id, zero_pt.x)                   0 fail -- an equivalent mutant: the only
      point of the curve with Z = 0 is (0 : y : 0), so X / Z' is 0 already; the two modules: 52 pass
  (b') its twin, without fe_cmov(a.y, id, zero_pt.y)                                       2 fail (both r2 tests); the two modules: 52 pass
  (c) agg_phase1_run's value-boundary step with sc_mul(ll, ll, lambda)                     28 of 38 fail
  (d) agg_c0_var with total = acc on every chunk                                           13 of 38 fail
So the verdict-level modules stay green when the k sums share a zeroed product or the identity comes out with a wrong y; the tests here
do not.  (The witness, r1 and msm tests are not touched by these four: none of them changes code those stages run.)  On the gcc build
an earlier version of the module (34 tests) failed 27, 0, 2, 27 and 12 under the same five."""
import random

import numpy as np
import pytest

import agg_cases as A
import agg_golden
import bppp_oracle as O
from prims import build as PB

P, NN = O.P, O.N
W = 4
SENT8, SENT32, SENT_STATUS = 0xEE, 0xEEEEEEEE, 7
SHAPES = [(3, 4, 4), (6, 2, 3), (7, 3, 4)]
NROWS = 71                     # 64 + 7: a second wavefront of 7 rows; 8 * 71 = 568 = 8 * 64 + 56 threads on the G = 8 grid
FB_L1, FB_LANES, FB_L64 = 0, 1, 2
TABLES = 0x100
V_NAMES = ("status", "tstate", "sc0", "pts", "acc", "pfix", "inv", "vsum", "commit", "c", "rho", "mu", "fell")


# the row classes whose variable-base sum takes the complete-formula fallback, per shape (expected_fell gives the mask of every row).  Equal
# or opposite points in a chunk meet an exceptional addition only where the accumulator holds the entry added or its negative, which the
# window digits of hash-derived scalars decide: at (3, 4, 4) no row of the batch does, and none of 399 further rows with c_l = c_s and
# c_r = j G did either, so that shape's fallback is entered by tests/test_prims.py's crafted sums only.
FELL = {(3, 4, 4): set(), (6, 2, 3): {"V2+R2=-(V1+R1)"}, (7, 3, 4): {"V2+R2=-(V1+R1)"}}


def form_of(G=1, fb=FB_LANES, tables=True):
    return G | (fb << 4) | (TABLES if tables else 0)


BACKEND_PARAMS = ["gcc", "clang", pytest.param("gfx950", marks=pytest.mark.gpu)]


@pytest.fixture(scope="module", params=BACKEND_PARAMS)
def backend(request):
    return request.param


_LIB, _TABLE, _BATCH, _EXP, _OUT = {}, {}, {}, {}, {}


def lib_of(backend):
    if backend not in _LIB:
        why = PB.unavailable(backend)
        if why:
            pytest.skip(f"{backend} backend skipped: {why}")
        _LIB[backend] = PB.load(backend)
    return _LIB[backend]


def table_of(backend, case):
    """fixed-base table of g | g_vec || g_vec_ | h_vec || h_vec_, built by the backend's own host code (prims_bucket_fb_build)"""
    key = (backend, case["k"], case["nd"])
    if key not in _TABLE:
        L = lib_of(backend)
        nb = 1 + case["NG"] + case["NH"]
        tab = np.zeros(L.prims_bucket_fb_entries(nb, W) * 64, np.uint8)
        assert L.prims_bucket_fb_build(agg_golden.generators(case), nb, W, tab.ctypes.data) == 0
        _TABLE[key] = tab
    return _TABLE[key]


# ---------------------------------------------------------------- the batch: one golden proof, one row per class
def xy(b):
    return np.frombuffer(bytes(b), np.uint8)


def neg(b):
    return xy(A.neg_point(bytes(b)))


def batch_of(shape):
    """(case, C [NROWS, k, 64], Q [NROWS, proof_bytes], {row: class name})"""
    if shape in _BATCH:
        return _BATCH[shape]
    case, coms, proofs, _ = agg_golden.load(shape)
    k, off = case["k"], A.field_offsets(case)
    R0 = off["R_first"]
    C, Q = np.repeat(coms[:1], NROWS, axis=0), np.repeat(proofs[:1], NROWS, axis=0)
    Rb = [proofs[0, R0 + 64 * i:R0 + 64 * i + 64].copy() for i in range(k)]
    Vb = [coms[0, i].copy() for i in range(k)]
    sums = [O.pt_add(O.pt_from_xy64(Vb[i].tobytes()), O.pt_from_xy64(Rb[i].tobytes())) for i in range(k)]
    cs = proofs[0, off["c_s"]:off["c_s"] + 64].copy()
    special = []

    def add(name, fn):
        special.append((name, fn))

    def setR(q, i, b):
        q[R0 + 64 * i:R0 + 64 * i + 64] = b

    def setf(q, name, b):
        q[off[name]:off[name] + 64] = b

    for i in sorted({0, k // 2, k - 1}):
        add(f"V{i}=R{i}", lambda c, q, i=i: c.__setitem__(i, Rb[i]))
    for i in range(k):
        add(f"V{i}=-R{i}", lambda c, q, i=i: c.__setitem__(i, neg(Rb[i])))

    def several(idx):
        def fn(c, q):
            for i in idx:
                c[i] = neg(Rb[i])
        return fn
    add("V=-R at two", several((0, k - 1)))
    add("V=-R at all", several(range(k)))
    add("V identity", lambda c, q: c.__setitem__(k // 2, 0))
    add("R identity", lambda c, q: setR(q, 1, 0))
    add("V and R identity", lambda c, q: (c.__setitem__(0, 0), setR(q, 0, 0)))

    def mix(c, q):
        c[0] = Rb[0]
        c[1] = neg(Rb[1])
        c[2] = 0
    add("mix", mix)
    # coincidences inside the first chunk (slots 0 .. 4: c_s, c_o, c_l, c_r, V_0 + R_0)
    add("c_l=c_s", lambda c, q: setf(q, "c_l", cs))
    add("c_o=-c_s", lambda c, q: setf(q, "c_o", neg(cs)))
    add("c_r=V0+R0", lambda c, q: setf(q, "c_r", xy(O.pt_to_xy64(sums[0]))))
    add("c_s identity", lambda c, q: setf(q, "c_s", 0))
    # across the chunk boundary (slot 5 = V_1 + R_1 and slot 0 = c_s), and inside the second chunk (V_1 + R_1, V_2 + R_2)
    add("V1+R1=c_s", lambda c, q: (c.__setitem__(1, cs), setR(q, 1, 0)))
    add("V2+R2=V1+R1", lambda c, q: (c.__setitem__(2, Vb[1]), setR(q, 2, Rb[1])))
    add("V2+R2=-(V1+R1)", lambda c, q: (c.__setitem__(2, neg(Vb[1])), setR(q, 2, neg(Rb[1]))))

    def off_curve(c, q):
        c[k // 2, 63] ^= 1
    add("V off the curve", off_curve)
    add("coordinate p", lambda c, q: q.__setitem__(slice(off["c_o"], off["c_o"] + 32), xy(P.to_bytes(32, "big"))))
    # special rows as neighbours (one lane group, one wavefront) from row 1 on, then honest rows between them, the last row special
    names = {}
    row = 1
    for j, (name, fn) in enumerate(special):
        fn(C[row], Q[row])
        names[row] = name
        row += 1 if j < 12 else 2
    assert row < 63
    for row, j in ((63, 4), (64, 0), (NROWS - 1, len(special) - 7)):      # both sides of the wavefront boundary, and the last row
        special[j][1](C[row], Q[row])
        names[row] = special[j][0]
    _BATCH[shape] = (case, C, Q, names)
    return _BATCH[shape]


# ---------------------------------------------------------------- what the oracle says of a row
class _C0Recorded(Exception):
    pass


class _TraceToC0(list):
    """the oracle's trace, stopped once the circuit verifier has recorded C0 (the WNLA stage behind it is not under test here)"""

    def extend(self, items):
        items = list(items)
        super().extend(items)
        if any(key == "C0" for key, _ in items):
            raise _C0Recorded


def state_words(t):
    """an oracle transcript in ws_st_strobe's words (verify_ws.h): the 200 state bytes as 50 little-endian words, pos, pos_begin"""
    st = t.strobe
    return np.frombuffer(bytes(st.state), "<u4").tolist() + [st.pos, st.pos_begin]


def expected_row(case, com, proof):
    """None for a row the oracle does not decode, else the dict of every value the stages store"""
    k, nd, np_ = case["k"], case["nd"], case["np"]
    tr = _TraceToC0()
    try:
        rc = A.verify(case, com, proof, tr)
        assert rc == -1 and not tr, "only a row that does not decode ends before C0"
        return None
    except _C0Recorded:
        pass
    d = dict(tr)
    e, rho, lam, delta, tau = d["e"], d["rho"], d["lambda"], d["delta"], d["tau"]
    mu = rho * rho % NN
    circ = A.make_circuit(case, e)
    var = [pow(tau, -1, NN), -delta % NN, tau, -tau * tau % NN]
    var += [2 * pow(tau, 3, NN) * circ.linear_comb_coef(i, lam, mu) % NN for i in range(k)]
    off = A.field_offsets(case)
    pts = [proof[off[n]:off[n] + 64] for n in ("c_s", "c_o", "c_l", "c_r")] + [O.pt_to_xy64(s) for s in d["V+R"]]
    pfix = O.pt_add(O.pt_mul(case["Pg"], d["ps_tau"]), O.vector_mul(case["Pgv"], d["pn_tau"], O.PT))
    acc = None
    for b, s in zip(pts, var):
        acc = O.pt_add(acc, O.pt_mul(O.pt_from_xy64(b), s))
    assert O.pt_add(pfix, acc) == d["C0"]
    # the transcript as phase 1 leaves it, behind the tau challenge: the oracle's own sequence once more, checked on its challenges
    t = O.Transcript(case["label"])
    for i in range(k):
        O.app_point(b"reciprocal_commitment", O.pt_from_xy64(com[64 * i:64 * i + 64]), t)
    assert O.get_challenge(b"reciprocal_challenge", t) == e
    for name, b in (("commitment_cl", pts[2]), ("commitment_cr", pts[3]), ("commitment_co", pts[1])):
        O.app_point(name.encode(), O.pt_from_xy64(b), t)
    for sm in d["V+R"]:
        O.app_point(b"commitment_v", sm, t)
    assert [O.get_challenge(b"circuit_" + n, t) for n in (b"rho", b"lambda", b"beta", b"delta")] == [rho, lam, d["beta"], delta]
    O.app_point(b"commitment_cs", O.pt_from_xy64(pts[0]), t)
    assert O.get_challenge(b"circuit_tau", t) == tau
    return dict(rho=rho, mu=mu, c=d["c"], sc0=[d["ps_tau"]] + d["pn_tau"] + var, inv=[pow(e + j, -1, NN) for j in range(np_)], pts=pts,
                sums=d["V+R"], pfix=pfix, acc=acc, c0=O.pt_to_xy64(d["C0"]), tstate=state_words(t))


# ---- which chunks of the variable-base sum meet an exceptional addition: straus_affine_fast's walk restated on the oracle's group law
# (straus_core.h: glv_decompose, glv_recode5, straus_affine_fast).  k = k1 + k2 lambda with the secp256k1 lattice constants below;
# each half as 26 signed 5-bit digits of |k| + sum_i 16 * 32^i; windows from the top, five doublings between them, in each window the
# streams k1 of P_0, k2 of phi(P_0), k1 of P_1, ...  The Jacobian accumulator's Z turns 0, and stays 0, exactly when an entry is added
# to an accumulator that holds the same point or its negative.
GLV_G1 = 0x3086D221A7D46BCDE86C90E49284EB153DAA8A1471E8CA7FE893209A45DBB031
GLV_G2 = 0xE4437ED6010E88286F547FA90ABFE4C4221208AC9DF506C61571B4AE8AC47F71
GLV_MB1 = 0xE4437ED6010E88286F547FA90ABFE4C3
GLV_MB2 = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFE8A280AC50774346DD765CDA83DB1562C
BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
OFF5 = sum(16 << (5 * i) for i in range(26))


def glv_halves(k):
    """[(|k1|, negative), (|k2|, negative)]"""
    c1, c2 = (k * GLV_G1 + (1 << 383)) >> 384, (k * GLV_G2 + (1 << 383)) >> 384
    r2 = (c1 * GLV_MB1 + c2 * GLV_MB2) % NN
    r1 = (k - r2 * O.LAMBDA) % NN
    assert (r1 + r2 * O.LAMBDA - k) % NN == 0
    out = []
    for r in (r1, r2):
        neg = r >= 1 << 129
        out.append((NN - r if neg else r, neg))
        assert out[-1][0] < 1 << 128
    return out


_MULT = {}


def small_multiple(pt, d):
    if (pt, d) not in _MULT:
        _MULT[(pt, d)] = O.pt_mul(pt, d)
    return _MULT[(pt, d)]


def chunk_meets_exception(points, scalars):
    streams = []
    for pt, k in zip(points, scalars):
        (a1, n1), (a2, n2) = glv_halves(k)
        streams.append((pt, a1 + OFF5, n1))
        streams.append((None if pt is None else (pt[0] * BETA % P, pt[1]), a2 + OFF5, n2))
    acc, empty = None, True
    for i in range(25, -1, -1):
        if not empty:
            for _ in range(5):
                acc = O.pt_add(acc, acc)
        for pt, w, sneg in streams:
            dg = ((w >> (5 * i)) & 31) - 16
            if dg == 0 or pt is None:
                continue
            e = small_multiple(pt, abs(dg))
            if (dg < 0) != sneg:
                e = O.pt_neg(e)
            if empty:
                acc, empty = e, False
                continue
            if acc is None or acc[0] == e[0]:
                return True
            acc = O.pt_add(acc, e)
    return False


def expected_fell(x):
    """bit c: chunk c (points 5 c .. 5 c + 4 of the 4 + k) takes the fallback"""
    pts = [O.pt_from_xy64(b) for b in x["pts"]]
    var = x["sc0"][-len(pts):]
    return sum(1 << c for c in range((len(pts) + 4) // 5) if chunk_meets_exception(pts[5 * c:5 * c + 5], var[5 * c:5 * c + 5]))


def expected(shape):
    if shape not in _EXP:
        case, C, Q, _ = batch_of(shape)
        memo = {}
        rows = []
        for r in range(NROWS):
            key = (C[r].tobytes(), Q[r].tobytes())
            if key not in memo:
                memo[key] = expected_row(case, *key)
                if memo[key] is not None:
                    memo[key]["fell"] = expected_fell(memo[key])
            rows.append(memo[key])
        _EXP[shape] = rows
    return _EXP[shape]


# ---------------------------------------------------------------- running and comparing
def run_verify(backend, shape, form):
    """every buffer of one call, transposed out of the [word][N] layout: name -> array with the instance first"""
    key = (backend, shape, form)
    if key in _OUT:
        return _OUT[key]
    L = lib_of(backend)
    case, C, Q, _ = batch_of(shape)
    k, nm, np_, NH, n = case["k"], case["nm"], case["np"], case["NH"], NROWS
    tab = table_of(backend, case)
    words = dict(tstate=52, sc0=(nm + 5 + k) * 8, pts=(4 + k) * 16, acc=30, pfix=30, inv=np_ * 8, vsum=k * 40)
    bufs = {"status": np.full(n, SENT_STATUS, np.int32)}
    for name, w in words.items():
        bufs[name] = np.full((w, n), SENT32, np.uint32)
    bufs.update(commit=np.full((n, 64), SENT8, np.uint8), c=np.full((n, NH, 32), SENT8, np.uint8), rho=np.full((n, 32), SENT8, np.uint8),
                mu=np.full((n, 32), SENT8, np.uint8), fell=np.full(n, SENT8, np.uint8))
    label = np.frombuffer(case["label"], np.uint8).copy()
    Cc, Qc = np.ascontiguousarray(C), np.ascontiguousarray(Q)
    dims = np.array([n, k, case["nd"], np_, case["rounds"], case["nl"], case["nn"], case["NG"], NH, form, W, len(label)], np.int64)
    vin = (PB.C.c_void_p * 4)(label.ctypes.data, tab.ctypes.data, Cc.ctypes.data, Qc.ctypes.data)
    vio = (PB.C.c_void_p * len(V_NAMES))(*[bufs[name].ctypes.data for name in V_NAMES])
    rc = L.run_agg_verify(dims.ctypes.data, vin, vio)
    assert rc == 0, f"{shape} form {form:#x} on {backend}: run returned {rc}"
    out = {name: (a.T.copy() if name in words else a) for name, a in bufs.items()}
    _OUT[key] = out
    return out


def words8(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def packed(b):
    """64 affine bytes -> the 16 packed words of ws_st_apt: x then y, least significant word first"""
    return words8(int.from_bytes(b[:32], "big")) + words8(int.from_bytes(b[32:], "big"))


def val26(col):
    return sum(int(l) << (26 * i) for i, l in enumerate(col))


def decode_point(w30):
    X, Y, Z = (val26(w30[10 * j:10 * j + 10]) % P for j in range(3))
    if Z == 0:
        return None
    zi = pow(Z, -1, P)
    p = (X * zi % P, Y * zi % P)
    assert O.on_curve(p)
    return p


def be(row):
    return int.from_bytes(row.tobytes(), "big")


def check(backend, shape, form, parts=("p1", "fixed", "var")):
    """the call's buffers against the oracle, row by row; returns them"""
    out = run_verify(backend, shape, form)
    case, _, _, names = batch_of(shape)
    exp = expected(shape)
    k = case["k"]
    for r in range(NROWS):
        what = f"{shape} form {form:#x} on {backend}, row {r} ({names.get(r, 'honest')})"
        x = exp[r]
        if x is None:
            assert out["status"][r] != SENT_STATUS and out["status"][r] & 1, what
            continue
        if "p1" in parts:
            assert out["status"][r] == 0, what
            assert be(out["rho"][r]) == x["rho"] and be(out["mu"][r]) == x["mu"], what
            assert [be(v) for v in out["c"][r]] == x["c"], what
            assert out["sc0"][r].tolist() == [w for s in x["sc0"] for w in words8(s)], what
            assert out["inv"][r].tolist() == [w for s in x["inv"] for w in words8(s)], what
            assert out["pts"][r].tolist() == [w for b in x["pts"] for w in packed(b)], what
            assert out["tstate"][r].tolist() == x["tstate"], what
            for i in range(k):      # vsum: per value 30 words of the projective sum, X | Y | Z, then 10 of the running product (agg_core.h: AggWs)
                assert (val26(out["vsum"][r][40 * i + 20:40 * i + 30]) % P == 0) == (x["sums"][i] is None), what
        if "fixed" in parts:
            assert decode_point(out["pfix"][r]) == x["pfix"], what
        if "var" in parts:
            assert decode_point(out["acc"][r]) == x["acc"], what
            assert out["commit"][r].tobytes() == x["c0"], what
            assert out["fell"][r] == (x["fell"] if form & TABLES else 0), what
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_batch_is_what_it_was_built_to_be(shape):
    """every row class is there, the oracle decodes all but the two malformed classes, and its sums are the identities the rows were made for"""
    case, C, Q, names = batch_of(shape)
    exp = expected(shape)
    k = case["k"]
    by = {}
    for r, name in names.items():
        by.setdefault(name, []).append(r)
    assert len(by) == len({0, k // 2, k - 1}) + k + 15 and NROWS - 1 in names and 63 in names and 64 in names
    assert sum(1 for r in range(NROWS) if r not in names) >= 20
    for r in range(NROWS):
        name = names.get(r, "honest")
        assert (exp[r] is None) == (name in ("V off the curve", "coordinate p")), name
    ids = lambda name: [i for i, s in enumerate(exp[by[name][0]]["sums"]) if s is None]
    assert ids("V=-R at all") == list(range(k)) and ids("V=-R at two") == [0, k - 1] and ids("mix") == [1] and ids("V and R identity") == [0]
    assert ids("V0=R0") == [] and ids("V identity") == [] and ids("R identity") == []
    x = exp[by["V1+R1=c_s"][0]]
    assert x["pts"][5] == x["pts"][0]
    x = exp[by["V2+R2=-(V1+R1)"][0]]
    assert x["pts"][6] == A.neg_point(x["pts"][5])


@pytest.mark.parametrize("G", (1, 2, 4, 8))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_phase1_on_every_lane_count(backend, shape, G):
    """k_agg_phase1 and k_agg_phase1_grp with 2, 4, 8 lanes: every value phase 1 stores, per row, against the oracle -- the k sums through
    one inversion with identities among them, the runs' powers across value boundaries ((7, 3, 4) on 8 lanes: runs of 3 entries, the
    last lane's run empty), cl_tau[nd] != 0 at (6, 2, 3)."""
    out = check(backend, shape, form_of(G=G), parts=("p1",))
    one = run_verify(backend, shape, form_of(G=1))
    for name in V_NAMES:
        assert (out[name] == one[name]).all(), f"{shape} G={G} on {backend}: {name} differs from the one-lane form's"


@pytest.mark.parametrize("fb", (FB_L1, FB_LANES, FB_L64), ids=("l1", "lanes", "l64"))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_fixed_base_half_on_every_kernel(backend, shape, fb):
    """k_agg_c0_fixed_l1, k_agg_c0_fixed and k_agg_c0_fixed_l64: pfix = ps_tau g + <g_vec, pn_tau> per row, and C0 behind it"""
    check(backend, shape, form_of(fb=fb), parts=("fixed", "var"))


@pytest.mark.parametrize("tables", (True, False), ids=("tables", "projective"))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_variable_base_half_on_both_forms(backend, shape, tables):
    """agg_c0_var over the window tables (chunks of five through straus_affine<M>, the chunk totals added) and over the projective tables:
    acc = the oracle's sum of the 4 + k terms and wn_commit = C0, with identity tables, equal and opposite points inside a chunk and on
    either side of a chunk boundary.  Which chunks take straus_affine<M>'s complete-formula fallback is asserted per row against the walk
    restated on the oracle (expected_fell); the rows that do are the fixed set FELL[shape], not empty at any shape."""
    out = check(backend, shape, form_of(tables=tables), parts=("var",))
    _, _, _, names = batch_of(shape)
    exp = expected(shape)
    if not tables:
        assert not out["fell"].any()
        return
    # (check() has compared the mask of every row with expected_fell's)
    fell = {names.get(r, "honest") for r in range(NROWS) if exp[r] is not None and exp[r]["fell"]}
    assert fell == FELL[shape], fell


def test_same_bytes_on_every_build(backend):
    """gcc, clang and gfx950 store identical words and bytes (acc and pfix are projective classes: compared as points above)."""
    others = [b for b in ("gcc", "clang") if b != backend and PB.unavailable(b) is None]
    if not others:
        pytest.skip("no second build to compare with")
    for shape in SHAPES:
        for form in (form_of(G=1), form_of(G=8), form_of(tables=False)):
            mine = run_verify(backend, shape, form)
            for other in others:
                theirs = run_verify(other, shape, form)
                for name in ("status", "sc0", "pts", "inv", "commit", "c", "rho", "mu", "fell", "tstate"):
                    assert (mine[name] == theirs[name]).all(), f"{shape} form {form:#x}: {name} differs between {backend} and {other}"


def test_arguments_out_of_range_are_refused(backend):
    """nothing runs for no instances, a lane count that is no power of two up to 8, an unknown fixed-base kernel or np > nd + 1"""
    L = lib_of(backend)
    case = batch_of(SHAPES[0])[0]
    good = [4, case["k"], case["nd"], case["np"], case["rounds"], case["nl"], case["nn"], case["NG"], case["NH"], form_of(), W, 4]
    null = (PB.C.c_void_p * 13)()
    for at, v in ((0, 0), (9, 3), (9, form_of(fb=3)), (3, case["nd"] + 2), (10, 8)):
        dims = np.array(good, np.int64)
        dims[at] = v
        assert L.run_agg_verify(dims.ctypes.data, null, null) != 0, (at, v)
    # the prover's: N, k, nd, np, NG, NH, stages, label_len -- no instances, np > nd + 1 behind the witness stage, k nd > NG, no stage,
    # an unknown stage bit, the msm without a table
    good = [4, 3, 4, 4, 16, 16, AGGP_R1, 4]
    for at, v in ((0, 0), (3, 6), (4, 8), (6, 0), (6, 32), (6, AGGP_MSM)):
        dims = np.array(good, np.int64)
        dims[at] = v
        assert L.run_agg_prove(dims.ctypes.data, null, null) != 0, (at, v)


# ---------------------------------------------------------------- the prover's stage r2 on crafted inputs
R2_N = 71
P_NAMES = ("x", "s", "rnd", "com", "digits", "m", "status", "row_status", "vsc", "tstate", "inst", "scr", "rsc", "rpb", "vsum", "cp_v", "cp_sv",
           "cp_wr", "cp_vpts", "proof_R")
AGGP_WITNESS, AGGP_R1, AGGP_MSM, AGGP_R2, AGGP_CT = 1, 2, 4, 8, 16


def run_prove(backend, n, k, nd, np_, NG, NH, stages, given, table=None):
    """one call of the prover entry point: every buffer pre-filled with the sentinel byte, `given` (name -> array) in place of it;
    returns name -> flat uint8 array (the given arrays themselves where given)"""
    L = lib_of(backend)
    rows, nm, nv = n * k, k * nd, nd + 1
    n_rnd = k + 18 + nv + nm
    sizes = dict(x=rows * 32, s=rows * 32, rnd=n * n_rnd * 32, com=rows * 64, digits=n * nm * 32, m=n * np_ * 32, status=n * 4,
                 row_status=rows * 4, vsc=64 * rows, tstate=208 * n, inst=(2 + np_) * 32 * n, scr=(nm + np_) * 32 * n, rsc=nv * 32 * rows,
                 rpb=120 * rows, vsum=k * 200 * n, cp_v=rows * nv * 32, cp_sv=rows * 32, cp_wr=n * nm * 32, cp_vpts=rows * 64, proof_R=rows * 64)
    bufs = {name: np.full(sz, SENT8, np.uint8) for name, sz in sizes.items()}
    for name, a in given.items():
        a = np.ascontiguousarray(a)
        assert a.nbytes == sizes[name], name
        bufs[name] = a
    label = np.frombuffer(b"aggregate test", np.uint8).copy()
    dims = np.array([n, k, nd, np_, NG, NH, stages, len(label)], np.int64)
    pin = (PB.C.c_void_p * 2)(label.ctypes.data, table.ctypes.data if table is not None else None)
    pio = (PB.C.c_void_p * len(P_NAMES))(*[bufs[name].ctypes.data for name in P_NAMES])
    rc = L.run_agg_prove(dims.ctypes.data, pin, pio)
    assert rc == 0, f"stages {stages} on {backend}: run returned {rc}"
    return bufs


def be_rows(a, per):
    """big-endian 32-byte scalars -> [[int] * per]"""
    v = [int.from_bytes(a[i:i + 32].tobytes(), "big") for i in range(0, a.size, 32)]
    return [v[i:i + per] for i in range(0, len(v), per)]


def word_rows(a, slots, cols):
    """a [slots * 8][cols] word array handed back as bytes -> [col][slot] integers"""
    w = a.view(np.uint32).reshape(slots * 8, cols)
    return [[sum(int(w[8 * sl + i, c]) << (32 * i) for i in range(8)) for sl in range(slots)] for c in range(cols)]


def be32(v):
    return v.to_bytes(32, "big")


# ---------------------------------------------------------------- the prover's witness stage
@pytest.mark.parametrize("shape", [(3, 5, 10), (6, 2, 3), (2, 16, 16)], ids=str)
def test_prover_witness_on_the_device_build(backend, shape):
    """k_aprove_witness at the edges of the range: 0, np^nd - 1, one above, n - 1 (canonical, out of range), n and n + 5 (not canonical), a
    non-canonical s; digits, multiplicities, status, row_status and the commitment scalars (zero on a flagged instance) against Python
    integers, 71 instances with the last one flagged."""
    k, nd, np_ = shape
    top, n = np_**nd, 71
    rg = random.Random(f"witness {shape}")
    xs = [[0] * k, [top - 1] * k, [top - 1] * (k - 1) + [top], [1] + [NN - 1] * (k - 1), [NN] + [3] * (k - 1), [NN + 5] + [top] * (k - 1)]
    xs += [[rg.randrange(top) for _ in range(k)] for _ in range(n - len(xs))]
    ss = [[rg.randrange(NN) for _ in range(k)] for _ in range(n)]
    ss[7][k - 1] = NN                       # a non-canonical s between honest rows, and in the last row
    ss[n - 1][0] = NN + 1
    x = np.frombuffer(b"".join(be32(v) for row in xs for v in row), np.uint8)
    s = np.frombuffer(b"".join(be32(v) for row in ss for v in row), np.uint8)
    out = run_prove(backend, n, k, nd, np_, 0, 0, AGGP_WITNESS, dict(x=x.copy(), s=s.copy()))
    dig, m = be_rows(out["digits"], k * nd), be_rows(out["m"], np_)
    st, rst = out["status"].view(np.int32), out["row_status"].view(np.int32).reshape(n, k)
    vsc = word_rows(out["vsc"], 2, n * k)
    for t in range(n):
        bad = any(v >= NN for v in xs[t] + ss[t])
        over = any(top <= v < NN for v in xs[t])
        want = (1 if bad else 0) | (4 if over else 0)
        assert st[t] == want and (rst[t] == want).all(), (shape, t, st[t], want)
        if all(v < NN for v in xs[t]):      # (a non-canonical x has no agreed digits; the instance is flagged)
            flat = [(v // np_**d) % np_ for v in xs[t] for d in range(nd)]
            assert dig[t] == flat and m[t] == [flat.count(v) for v in range(np_)], (shape, t)
        for i in range(k):
            assert vsc[t * k + i] == ([xs[t][i], ss[t][i]] if want == 0 else [0, 0]), (shape, t, i)
    assert (out["cp_v"] == SENT8).all() and (out["rsc"] == SENT8).all()


# ---------------------------------------------------------------- the prover's stage r1 on the witness kernel's output
_POOL = {}


def pool_point(j):
    if j not in _POOL:
        _POOL[j] = O.pt_mul(O.G, 0xA66 + 977 * j)
    return _POOL[j]


@pytest.mark.parametrize("shape", [(6, 2, 3), (7, 3, 4)], ids=str)
def test_prover_stage_r1_values(backend, shape):
    """k_aprove_witness then k_aprove_stage_r1: e from the oracle's transcript over the k commitments; cp_wr = (digit + e)^-1, cp_v =
    [x_i, r_i...], cp_sv = s_i + rb_i, rsc = rb_i | r_{i,d} (value-major rows, filled by the reversed walk of (vi, d)), inst_vals = -e |
    -(e + j)^-1 as big integers, tstate the oracle's state behind the challenge.  One row's rnd holds rb = n (status & 1), one row is
    flagged by the witness (a value one above the range: its status passes through).  digit + e = 0 cannot be constructed -- e is a hash
    output -- so the substituted-zero branch of the inversion is not entered here."""
    k, nd, np_ = shape
    case = A.setup(k, nd, np_)
    n, nm, nv, top = 71, k * nd, nd + 1, np_**nd
    n_rnd = k + 18 + nv + nm
    rg = random.Random(f"r1 {shape}")
    xs = [[rg.randrange(top) for _ in range(k)] for _ in range(n)]
    xs[0], xs[1] = [0] * k, [top - 1] * k
    OVER, BAD_RB = 9, 66
    xs[OVER][k // 2] = top
    ss = [[rg.randrange(NN) for _ in range(k)] for _ in range(n)]
    rb = [[rg.randrange(NN) for _ in range(k)] for _ in range(n)]
    rb[2][0], rb[3][k - 1] = 0, NN - 1
    rnd = np.full((n, n_rnd, 32), 0x11, np.uint8)
    for t in range(n):
        for i in range(k):
            rnd[t, i] = xy(be32(rb[t][i]))
    rnd[BAD_RB, 1] = xy(be32(NN))
    V = [[pool_point(rg.randrange(16)) for _ in range(k)] for _ in range(n)]
    V[4][0] = V[4][1]
    V[OVER] = [None] * k                    # (what the commitment kernels leave for a flagged instance: identities)
    com = np.frombuffer(b"".join(O.pt_to_xy64(p) for row in V for p in row), np.uint8).copy()
    x = np.frombuffer(b"".join(be32(v) for row in xs for v in row), np.uint8).copy()
    s = np.frombuffer(b"".join(be32(v) for row in ss for v in row), np.uint8).copy()
    out = run_prove(backend, n, k, nd, np_, case["NG"], case["NH"], AGGP_WITNESS | AGGP_R1, dict(x=x, s=s, rnd=rnd, com=com))
    st = out["status"].view(np.int32)
    wr, cpv, sv = be_rows(out["cp_wr"], nm), be_rows(out["cp_v"], nv), be_rows(out["cp_sv"], 1)
    rsc, inst = word_rows(out["rsc"], nv, n * k), word_rows(out["inst"], 2 + np_, n)
    ts = out["tstate"].view(np.uint32).reshape(52, n)
    for t in range(n):
        what = f"{shape} on {backend}, instance {t}"
        tr = O.Transcript(case["label"])
        for p in V[t]:
            O.app_point(b"reciprocal_commitment", p, tr)
        e = O.get_challenge(b"reciprocal_challenge", tr)
        assert ts[:, t].tolist() == state_words(tr), what
        r = [[pow((xs[t][i] // np_**d) % np_ + e, -1, NN) for d in range(nd)] for i in range(k)]
        assert wr[t] == [a for row in r for a in row], what
        assert inst[t][:1 + np_] == [-e % NN] + [-pow(e + j, -1, NN) % NN for j in range(np_)], what
        assert inst[t][1 + np_] == int.from_bytes(bytes([SENT8]) * 32, "little"), what      # (mu^-1's slot: the collect's, not this stage's)
        if t == BAD_RB:
            assert st[t] & 1, what
            continue
        assert st[t] == (4 if t == OVER else 0), what
        for i in range(k):
            row = t * k + i
            assert cpv[row] == [xs[t][i]] + r[i], what
            assert sv[row] == [(ss[t][i] + rb[t][i]) % NN], what
            assert rsc[row] == [rb[t][i]] + r[i], what


# ---------------------------------------------------------------- the pole commitments' sum over N k rows
@pytest.mark.parametrize("ct", (0, 1))
def test_prover_pole_commitment_sum(backend, ct):
    """k_aprove_msm: rpb, brought to affine, = rb_i h_vec[0] + sum_d r_{i,d} h_vec[9 + d] on the plain and on the constant-time lookups.
    23 x 3 = 69 rows: three blocks of 32 rows, the last one ragged; a row of all-zero scalars (the identity), a row with rb = n - 1, rows of
    small and of top scalars."""
    case = A.setup(3, 4, 4)
    k, nd, np_, n = 3, 4, 4, 23
    rows, nv = n * k, nd + 1
    rg = random.Random("poles")
    sc = [[rg.randrange(NN) for _ in range(nv)] for _ in range(rows)]
    sc[5] = [0] * nv
    sc[6] = [NN - 1] + sc[6][1:]
    sc[31], sc[32] = [1] * nv, [NN - 1] * nv
    sc[rows - 1] = [0, 0, 0, 0, 7]
    rsc = np.zeros((nv * 8, rows), np.uint32)
    for row in range(rows):
        rsc[:, row] = [w for v in sc[row] for w in words8(v)]
    out = run_prove(backend, n, k, nd, np_, case["NG"], case["NH"], AGGP_MSM | (AGGP_CT if ct else 0), dict(rsc=rsc.view(np.uint8).reshape(-1)),
                    table=table_of(backend, case))
    rpb = out["rpb"].view(np.uint32).reshape(30, rows)
    hv = case["Phv"]
    for row in range(rows):
        e = O.pt_mul(hv[0], sc[row][0])
        for d in range(nd):
            e = O.pt_add(e, O.pt_mul(hv[9 + d], sc[row][1 + d]))
        assert decode_point(rpb[:, row]) == e, f"ct={ct} on {backend}: row {row}"
    assert decode_point(rpb[:, 5]) is None
    assert (out["proof_R"] == SENT8).all()


def limbs26(x):
    return [(x >> (26 * i)) & 0x3FFFFFF for i in range(9)] + [x >> 234]


def r2_case(k):
    """(V logs [N][k], R logs [N][k]) with 0 for the identity: the row classes of stage r2, honest rows between them, the last row special"""
    rg = random.Random(f"r2 {k}")
    V = [[rg.randrange(1, NN) for _ in range(k)] for _ in range(R2_N)]
    R = [[rg.randrange(1, NN) for _ in range(k)] for _ in range(R2_N)]
    classes = []
    for i in sorted({0, k // 2, k - 1}):
        classes.append({i: "eq"})
        classes.append({i: "neg"})
    classes += [{0: "neg", k - 1: "neg"}, {i: "neg" for i in range(k)}, {k // 2: "V0"}, {1: "R0"}, {0: "00"}, {i: "00" for i in range(k)},
                {0: "eq", 1: "neg", 2: "V0"}, {i: "R0" for i in range(k)}]
    rows = list(range(1, 1 + len(classes))) + [63, 64, R2_N - 1]
    for row, cl in zip(rows, classes + [classes[7], classes[1], classes[11]]):
        for i, what in cl.items():
            if what == "eq":
                V[row][i] = R[row][i]
            elif what == "neg":
                V[row][i] = NN - R[row][i]
            if what in ("V0", "00"):
                V[row][i] = 0
            if what in ("R0", "00"):
                R[row][i] = 0
    return V, R


@pytest.mark.parametrize("k", (3, 7))
def test_prover_stage_r2_on_exceptional_sums(backend, k):
    """k_aprove_stage_r2: R_i (projective, a random Z each; (0 : y : 0) for the identity) and V_i + R_i by the complete law to affine
    through ONE field inversion.  Rows: generic, V_i = R_i, V_i = -R_i at one, two and all i, V_i the identity, R_i the identity, both, all
    2 k points identities, and all R_i identities; cp_vpts and proof_R are the oracle's affine bytes in every row, the generic neighbours
    included."""
    L = lib_of(backend)
    nd, np_ = 3, 4
    NG, NH = 32, 16
    n, rows = R2_N, R2_N * k
    V, R = r2_case(k)
    rg = random.Random(f"r2 z {k}")
    mul = lambda lg: O.pt_mul(O.G, lg) if lg else None
    com = np.zeros((rows, 64), np.uint8)
    rpb = np.zeros((30, rows), np.uint32)
    e_vp, e_R = [], []
    for t in range(n):
        for i in range(k):
            pv, pr = mul(V[t][i]), mul(R[t][i])
            com[t * k + i] = xy(O.pt_to_xy64(pv))
            z = rg.randrange(1, P)
            X, Y, Z = (0, z, 0) if pr is None else (pr[0] * z % P, pr[1] * z % P, z)
            rpb[:, t * k + i] = limbs26(X) + limbs26(Y) + limbs26(Z)
            e_vp.append(O.pt_to_xy64(O.pt_add(pv, pr)))
            e_R.append(O.pt_to_xy64(pr))
    bufs = run_prove(backend, n, k, nd, np_, NG, NH, AGGP_R2, dict(com=com.reshape(-1), rpb=rpb.view(np.uint8).reshape(-1)))
    got_vp, got_R = bufs["cp_vpts"].reshape(rows, 64), bufs["proof_R"].reshape(rows, 64)
    for r in range(rows):
        what = f"k={k} on {backend}: instance {r // k}, value {r % k}"
        assert got_vp[r].tobytes() == e_vp[r], what
        assert got_R[r].tobytes() == e_R[r], what
    for name in ("status", "digits", "cp_v", "cp_wr", "rsc"):      # (what the stage does not write stays as it was)
        assert (bufs[name] == SENT8).all(), name
    assert (bufs["com"].reshape(rows, 64) == com).all() and (bufs["rpb"].view(np.uint32).reshape(30, rows) == rpb).all()
