"""The generic ArithmeticCircuit verifier's phase 1 and C0 stage (circuit_core.h, k_generic.hip: k_circuit_*) on their RESULTS, not on
verdicts, over the shape family of tests/circuit_cases.py, on the three builds of tests/prims:

  gcc, clang  the host builds: the single-thread form (circuit_phase1, fb_sum_serial over the plan's lane count, circuit_c0_tables / var /
              finish) -- the window-table and the projective-table form of the variable-base sum
  gfx950      marked gpu: the product's own kernels -- tests/prims/circuit_device.hip includes bp_pp_amd/csrc/k_generic.hip as it is and
              launches k_circuit_phase1, k_circuit_c0_fixed[_l64], one of the three forms of the variable-base sum (k_circuit_c0_var_pts on
              plan_generic's c0_lanes; k_circuit_c0_tables + k_circuit_c0_var; k_circuit_c0_var without tables) and k_circuit_c0_finish
              with the grids of circuit_verify_host_impl

Where the reference rejects its own prover's output (circuit_cases.COMPLETE) the verdict-level tests compare 0 with 0: a phase 1 that
wrote a wrong c, or a C0 stage that dropped a chunk or a lane, passes them.  Here a batch of 67 rows per statement (5 for k60, k61 and
nm16, whose point is the group width) -- honest rows, a tampered scalar, a swapped commitment, a coordinate equal to p, an off-curve
point in the last row; a second wavefront with a ragged end in the one-lane grids, and 67 L threads that do not fill their last block for
L = 8, 16, 32 -- is compared per row, all exact, with the trace of bppp_oracle.ArithmeticCircuit.verify (stopped once C0 is recorded)
and with big integers:

  bit for bit   status, wn_rho, wn_mu, all NH entries of wn_c, lambda_vec, mu_vec, the six coefficient vectors, sc0 (ps_tau | pn_tau |
                tau^-1, -delta, tau, -tau^2 | 2 tau^3 coef_i), pts, the transcript state behind circuit_tau, wn_commit = C0
  as points     pfix = ps_tau g + <g_vec, pn_tau>, acc = the sum of the 4 + k terms
  between forms acc as a group element and wn_commit byte for byte

A malformed row runs on identity points: its status bit and its wn_c (the oracle's c over identity points) are compared, nothing else.
The rows are drawn from at most 6 distinct oracle instances per statement (three honest ones, the swapped commitment, the two malformed).

Measured: the CPU tier (gcc and clang, 132 tests plus the 16 batch checks) 40 s for this module, its slowest test 2.6 s; on an MI355X the
module's 66 gfx950 tests take 7.1 s, the slowest 1.0 s (test_same_bytes_on_every_build, which also runs a host build), the slowest that
only runs kernels 0.6 s (k60 on 64 lanes per instance).

One-line mutants of circuit_core.h, applied one at a time outside the tree:
  (a) circuit_c0_var without its last chunk (both branches), gcc build: this module fails at every statement with more than five points
      (k4, k5, k11, k13, k60, k61, nv8, fm_nv2, fl_fm, fl_fm_k5, mixed_k2) and passes at the one-chunk shapes (nm5 .. nm16) and at `nof`,
      whose last chunk holds a point under a zero scalar -- there the mutant is equivalent; tests/test_circuit_emul.py fails at the same ones
  (b) circuit_c0_var_points with `m < 8` for `m < L` in the shuffle loop, gfx950 on an MI355X: the lane-per-point case and test_forms_agree
      fail at k5, k11, k13, k60 and fl_fm_k5 (L = 16, 16, 32, 64, 16), 10 of 66; every L = 8 statement passes
  (c) circuit_phase1 without the `j < nv - 1` guard, gcc build: fails at every statement with a flag set, nv > 1 (k4, nv8, nm5 .. nm16,
      mixed_k2, and the incomplete fm_nv2, fl_fm) as well as nv = 1 (k5 .. k61, fl_fm_k5: the guard is all that keeps the single entry);
      `nof` passes, as it must: with neither flag the guard guards nothing."""
import numpy as np
import pytest

import bppp_oracle as O
import circuit_cases
from prims import build as PB

P, NN = O.P, O.N
W = 4
SENT8, SENT32, SENT_STATUS = 0xEE, 0xEEEEEEEE, 7
POINTS, TABLES, PROJECTIVE = 0, 1, 2
FORM_IDS = {POINTS: "points", TABLES: "tables", PROJECTIVE: "projective"}
NAMES = list(circuit_cases.FAMILY) + ["mixed_k2", "fl_fm"]
SMALL = {"k60", "k61", "nm16"}
IN_NAMES = ("label", "table", "com", "proofs", "Wm", "Wl", "am", "al", "LO", "LL", "LR", "NO")
BUF_NAMES = ("status", "tstate", "lamv", "muv", "coef", "sc0", "pts", "acc", "pfix", "commit", "c", "rho", "mu", "plan")
MALFORMED = ("coordinate p", "V off the curve")

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


def nrows(name):
    return 5 if name in SMALL else 67


def forms_of(backend, name):
    """the forms of the variable-base sum a build runs at a statement: the lane-per-point form on the device, up to 64 points"""
    per_point = backend == "gfx950" and circuit_cases.c0_lanes(name) <= 64
    return ([POINTS] if per_point else []) + [TABLES, PROJECTIVE]


# ---------------------------------------------------------------- the batch
def batch_of(name):
    """(case, C [n, k, 64], Q [n, proof_bytes], {row: class name}): honest rows from three instances, the special rows between them"""
    if name in _BATCH:
        return _BATCH[name]
    case = circuit_cases.make(name, 3)
    n, k = nrows(name), case["k"]
    C = np.stack([case["commitments"][r % 3] for r in range(n)])
    Q = np.stack([case["proofs"][r % 3] for r in range(n)])

    def tampered(c, q):
        q[-1] ^= 1

    def swapped(c, q):
        c[:] = case["commitments"][1]
        q[:] = case["proofs"][1]
        c[0] = case["commitments"][0, 0]

    def coordinate_p(c, q):
        q[128:160] = np.frombuffer(P.to_bytes(32, "big"), np.uint8)      # c_o's x

    def off_curve(c, q):
        c[k - 1, 63] ^= 1

    classes = {"tampered scalar": tampered, "swapped commitment": swapped, "coordinate p": coordinate_p, "V off the curve": off_curve}
    if n == 5:
        where = {1: "tampered scalar", 2: "swapped commitment", 3: "coordinate p", 4: "V off the curve"}
    else:      # neighbours in one lane group, both sides of the wavefront boundary, the last row
        where = {1: "tampered scalar", 2: "swapped commitment", 3: "coordinate p", 9: "V off the curve", 63: "swapped commitment",
                 64: "coordinate p", 65: "tampered scalar", n - 1: "V off the curve"}
    for row, cl in where.items():
        classes[cl](C[row], Q[row])
    _BATCH[name] = (case, C, Q, where)
    return _BATCH[name]


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


def oracle_circuit(case):
    pts = lambda lst: [O.pt_from_xy64(b) for b in lst]
    part = lambda typ, j: (None if case["part"][typ][j] < 0 else case["part"][typ][j])
    return O.ArithmeticCircuit(dim_nm=case["nm"], dim_no=case["no"], k=case["k"], dim_nl=case["nl"], dim_nv=case["nv"], dim_nw=case["nw"],
                               g=O.pt_from_xy64(case["g"]), g_vec=pts(case["gv"]), h_vec=pts(case["hv"]), W_m=case["W_m"], W_l=case["W_l"],
                               a_m=case["a_m"], a_l=case["a_l"], f_l=case["f_l"], f_m=case["f_m"], g_vec_=pts(case["gv_"]),
                               h_vec_=pts(case["hv_"]), partition=part)


def state_words(t):
    """an oracle transcript in ws_st_strobe's words (verify_ws.h): the 200 state bytes as 50 little-endian words, pos, pos_begin"""
    st = t.strobe
    return np.frombuffer(bytes(st.state), "<u4").tolist() + [st.pos, st.pos_begin]


def decodes(b):
    try:
        O.pt_from_xy64(b)
    except ValueError:
        return False
    return int.from_bytes(b[:32], "big") < P and int.from_bytes(b[32:], "big") < P


def expected_row(case, circ, com, head):
    """com: the k commitments' bytes, head: c_l | c_r | c_o | c_s (the proof's first 256 bytes).  A dict of every value the stages store;
    for a row that does not decode only `c` (over identity points, as the kernel runs it) and malformed = True"""
    k = case["k"]
    blobs = [head[64 * i:64 * i + 64] for i in range(4)] + [com[64 * i:64 * i + 64] for i in range(k)]
    malformed = not all(decodes(b) for b in blobs)
    if malformed:
        blobs = [bytes(64)] * (4 + k)
    cl, cr, co, cs = (O.pt_from_xy64(b) for b in blobs[:4])
    V = [O.pt_from_xy64(b) for b in blobs[4:]]
    proof = O.CircuitProof(c_l=cl, c_r=cr, c_o=co, c_s=cs, r=[], x=[], l=[], n=[])
    tr = _TraceToC0()
    try:
        circ.verify(V, O.Transcript(case["label"]), proof, tr)
        raise AssertionError("the trace ends with C0")
    except _C0Recorded:
        pass
    d = dict(tr)
    if malformed:
        return dict(malformed=True, c=d["c"])
    rho, lam, beta, delta, tau = d["rho"], d["lambda"], d["beta"], d["delta"], d["tau"]
    mu = rho * rho % NN
    lambda_vec = circ.collect_lambda(lam, mu)
    mu_vec = O.vector_mul_on_scalar(O.e_vec(mu, case["nm"]), mu)
    coef = [x for vec in circ.collect_c(lambda_vec, mu_vec, mu) for x in vec]
    var = [pow(tau, -1, NN), -delta % NN, tau, -tau * tau % NN]
    var += [2 * pow(tau, 3, NN) * circ.linear_comb_coef(i, lam, mu) % NN for i in range(k)]
    order = [blobs[3], blobs[2], blobs[0], blobs[1]] + blobs[4:]      # c_s, c_o, c_l, c_r, v_0 ..
    pfix = O.pt_add(O.pt_mul(circ.g, d["ps_tau"]), O.vector_mul(circ.g_vec, d["pn_tau"], O.PT))
    acc = None
    for b, s in zip(order, var):
        acc = O.pt_add(acc, O.pt_mul(O.pt_from_xy64(b), s))
    assert O.pt_add(pfix, acc) == d["C0"]
    # the transcript as phase 1 leaves it, behind the tau challenge: the oracle's own sequence once more, checked on its challenges
    t = O.Transcript(case["label"])
    for name, p in ((b"commitment_cl", cl), (b"commitment_cr", cr), (b"commitment_co", co)):
        O.app_point(name, p, t)
    for p in V:
        O.app_point(b"commitment_v", p, t)
    assert [O.get_challenge(b"circuit_" + n, t) for n in (b"rho", b"lambda", b"beta", b"delta")] == [rho, lam, beta, delta]
    O.app_point(b"commitment_cs", cs, t)
    assert O.get_challenge(b"circuit_tau", t) == tau
    return dict(malformed=False, rho=rho, mu=mu, c=d["c"], lamv=lambda_vec, muv=mu_vec, coef=coef, sc0=[d["ps_tau"]] + d["pn_tau"] + var,
                pts=order, pfix=pfix, acc=acc, c0=O.pt_to_xy64(d["C0"]), tstate=state_words(t))


def expected(name):
    if name not in _EXP:
        case, C, Q, _ = batch_of(name)
        circ = oracle_circuit(case)
        memo, rows = {}, []
        for r in range(C.shape[0]):
            key = (C[r].tobytes(), Q[r, :256].tobytes())      # (nothing behind the four points is read by these stages)
            if key not in memo:
                memo[key] = expected_row(case, circ, *key)
            rows.append(memo[key])
        assert len(memo) <= 8
        _EXP[name] = rows
    return _EXP[name]


# ---------------------------------------------------------------- running and comparing
def table_of(backend, name, case):
    key = (backend, name)
    if key not in _TABLE:
        L = lib_of(backend)
        gens = case["g"] + b"".join(case["gv"]) + b"".join(case["gv_"]) + b"".join(case["hv"]) + b"".join(case["hv_"])
        nb = 1 + case["NG"] + case["NH"]
        tab = np.zeros(L.prims_bucket_fb_entries(nb, W) * 64, np.uint8)
        assert L.prims_bucket_fb_build(gens, nb, W, tab.ctypes.data) == 0
        _TABLE[key] = tab
    return _TABLE[key]


def call(backend, name, form, n=None):
    """(return code, buffers) of one call"""
    L = lib_of(backend)
    case, C, Q, _ = batch_of(name)
    n = C.shape[0] if n is None else n
    nm, nv, k, nl, NH = case["nm"], case["nv"], case["k"], case["nl"], case["NH"]
    words = dict(tstate=52, lamv=nl * 8, muv=nm * 8, coef=(3 * nm + 3 * nv) * 8, sc0=(nm + 5 + k) * 8, pts=(4 + k) * 16, acc=30, pfix=30)
    bufs = {"status": np.full(n, SENT_STATUS, np.int32)}
    for nm_, w in words.items():
        bufs[nm_] = np.full((w, n), SENT32, np.uint32)
    bufs.update(commit=np.full((n, 64), SENT8, np.uint8), c=np.full((n, NH, 32), SENT8, np.uint8), rho=np.full((n, 32), SENT8, np.uint8),
                mu=np.full((n, 32), SENT8, np.uint8), plan=np.full(6, -1, np.int32))
    u8 = lambda b: np.frombuffer(b, np.uint8).copy() if len(b) else np.zeros(1, np.uint8)
    ins = dict(label=u8(case["label"]), table=table_of(backend, name, case), com=np.ascontiguousarray(C[:n]), proofs=np.ascontiguousarray(Q[:n]),
               Wm=u8(case["Wm_bytes"]), Wl=u8(case["Wl_bytes"]), am=u8(case["am_bytes"]), al=u8(case["al_bytes"]),
               **{t: np.ascontiguousarray(case["parts"][t]) for t in circuit_cases.TYPES})
    dims = np.array([n, nm, case["no"], nv, k, int(case["f_l"]), int(case["f_m"]), case["rounds"], case["pl"], case["pn"], case["NG"], NH, form, W,
                     len(case["label"])], np.int64)
    vin = (PB.C.c_void_p * len(IN_NAMES))(*[ins[x].ctypes.data for x in IN_NAMES])
    vio = (PB.C.c_void_p * len(BUF_NAMES))(*[bufs[x].ctypes.data for x in BUF_NAMES])
    rc = L.run_circuit(dims.ctypes.data, vin, vio)
    return rc, {x: (a.T.copy() if x in words else a) for x, a in bufs.items()}


def run(backend, name, form):
    """every buffer of one call, transposed out of the [word][N] layout: name -> array with the instance first"""
    key = (backend, name, form)
    if key not in _OUT:
        rc, out = call(backend, name, form)
        assert rc == 0, f"{name} form {FORM_IDS[form]} on {backend}: run returned {rc}"
        _OUT[key] = out
    return _OUT[key]


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


def flat8(vals):
    return [w for s in vals for w in words8(s % NN)]


def check(backend, name, form):
    out = run(backend, name, form)
    case, C, _, where = batch_of(name)
    exp = expected(name)
    L = circuit_cases.c0_lanes(name)
    assert out["plan"][:2].tolist() == [L, 1 if L <= 64 else 0], f"{name}: the plan's c0_lanes, per_point"
    for r in range(C.shape[0]):
        what = f"{name} form {FORM_IDS[form]} on {backend}, row {r} ({where.get(r, 'honest')})"
        x = exp[r]
        assert x["malformed"] == (where.get(r) in MALFORMED), what
        assert [be(v) for v in out["c"][r]] == x["c"] and len(x["c"]) == case["NH"], what
        if x["malformed"]:
            assert out["status"][r] != SENT_STATUS and out["status"][r] & 1, what
            continue
        assert out["status"][r] == 0, what
        assert be(out["rho"][r]) == x["rho"] and be(out["mu"][r]) == x["mu"], what
        assert out["lamv"][r].tolist() == flat8(x["lamv"]), what
        assert out["muv"][r].tolist() == flat8(x["muv"]), what
        assert out["coef"][r].tolist() == flat8(x["coef"]), what
        assert out["sc0"][r].tolist() == flat8(x["sc0"]), what
        assert out["pts"][r].tolist() == [w for b in x["pts"] for w in packed(b)], what
        assert out["tstate"][r].tolist() == x["tstate"], what
        assert decode_point(out["pfix"][r]) == x["pfix"], what
        assert decode_point(out["acc"][r]) == x["acc"], what
        assert out["commit"][r].tobytes() == x["c0"], what
    return out


@pytest.mark.parametrize("name", NAMES)
def test_batch_is_what_it_was_built_to_be(name):
    """every row class is there, the last row is the off-curve one, the oracle decodes all but the two malformed classes, the zero tail
    of c is as long as NH says, and a statement without a flag has k zero scalars"""
    case, C, Q, where = batch_of(name)
    exp = expected(name)
    n = C.shape[0]
    assert set(where.values()) == {"tampered scalar", "swapped commitment", "coordinate p", "V off the curve"}
    assert where[n - 1] == "V off the curve" and n - len(where) >= 1
    for r in range(n):
        assert exp[r]["malformed"] == (where.get(r) in MALFORMED)
        assert exp[r]["c"][9 + case["nv"]:] == [0] * (case["NH"] - 9 - case["nv"])
    honest = exp[0]
    assert (honest["sc0"][-case["k"]:] == [0] * case["k"]) == (not case["f_l"] and not case["f_m"])
    swapped = exp[[r for r, cl in where.items() if cl == "swapped commitment"][0]]
    assert swapped["c0"] != exp[1 if n == 5 else 4]["c0"] and swapped["pts"][4] == honest["pts"][4]


def _cases(forms):
    return [(name, form) for name in NAMES for form in forms]


@pytest.mark.parametrize("name,form", _cases((POINTS, TABLES, PROJECTIVE)), ids=lambda v: FORM_IDS.get(v, v) if isinstance(v, int) else v)
def test_stage_values_vs_oracle(backend, name, form):
    """phase 1, the fixed-base half, one form of the variable-base sum and the finish, every stored value per row against the oracle.
    A form a build cannot run is refused by the launcher, and that is asserted: the lane-per-point form on the host, and past 64 points."""
    if form not in forms_of(backend, name):
        rc, out = call(backend, name, form, n=2)
        assert rc != 0 and (out["status"] == SENT_STATUS).all() and (out["commit"] == SENT8).all()
        return
    check(backend, name, form)


@pytest.mark.parametrize("name", NAMES)
def test_forms_agree(backend, name):
    """the forms of the variable-base sum agree on acc as a group element and on wn_commit byte for byte, and on everything in front of
    the sum bit for bit (the malformed rows aside: nothing downstream of their status is specified)"""
    exp = expected(name)
    good = [r for r, x in enumerate(exp) if not x["malformed"]]
    forms = forms_of(backend, name)
    first = run(backend, name, forms[0])
    for form in forms[1:]:
        other = run(backend, name, form)
        for x in ("status", "tstate", "lamv", "muv", "coef", "sc0", "pts", "c", "rho", "mu"):
            assert (first[x] == other[x]).all(), (name, x)
        for r in good:
            assert decode_point(first["acc"][r]) == decode_point(other["acc"][r]), (name, r)
            assert first["commit"][r].tobytes() == other["commit"][r].tobytes(), (name, r)
            assert decode_point(first["pfix"][r]) == decode_point(other["pfix"][r]), (name, r)


def test_same_bytes_on_every_build(backend):
    """gcc, clang and gfx950 store identical words and bytes (acc and pfix are projective classes: compared as points above)."""
    others = [b for b in ("gcc", "clang") if b != backend and PB.unavailable(b) is None]
    if not others:
        pytest.skip("no second build to compare with")
    for name in ("k5", "k13", "nv8", "fl_fm_k5"):
        mine = run(backend, name, TABLES)
        theirs = run(others[0], name, TABLES)
        good = [r for r, x in enumerate(expected(name)) if not x["malformed"]]
        for x in ("status", "c", "rho", "mu", "tstate", "lamv", "muv", "coef", "sc0", "pts"):
            assert (mine[x] == theirs[x]).all(), (name, x)
        assert (mine["commit"][good] == theirs["commit"][good]).all(), name


def test_arguments_out_of_range_are_refused(backend):
    """nothing runs for no instances, an unknown form, nm > NG, nv + 9 > NH, a table width the launcher has no table for"""
    L = lib_of(backend)
    case = batch_of("k4")[0]
    good = [4, case["nm"], case["no"], case["nv"], case["k"], 1, 0, case["rounds"], case["pl"], case["pn"], case["NG"], case["NH"], TABLES, W, 4]
    null_in, null_io = (PB.C.c_void_p * len(IN_NAMES))(), (PB.C.c_void_p * len(BUF_NAMES))()
    for at, v in ((0, 0), (12, 3), (1, case["NG"] + 1), (3, case["NH"] - 8), (13, 8), (4, 125)):
        dims = np.array(good, np.int64)
        dims[at] = v
        assert L.run_circuit(dims.ctypes.data, null_in, null_io) != 0, (at, v)
