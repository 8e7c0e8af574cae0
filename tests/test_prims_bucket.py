"""The bucket (Pippenger) stage of the RLC batch mode on its RESULTS, not on verdicts: bkt_prepare, the left-hand side of
k_bkt_accumulate (LDS counting sort, lane-owned buckets, suffix scan, shuffle trees, Horner over the windows), the combined scalars of
k_bkt_scalars (unreduced 12-limb sums through a carry-propagating shuffle tree) and the verdict of k_bkt_check (fb_group_sum<64>),
against big integers and the Python oracle's group law, on the three builds of tests/prims:

  gcc, clang  the host builds: the single-thread form of bucket_core.h (bkt_prepare, bkt_superchunk_serial)
  gfx950      marked gpu: the product's own kernels -- tests/prims/bucket_device.hip includes bp_pp_amd/csrc/k_verify_bucket.hip as it is
              and launches it with launch_bucket_stage's geometry (bucket_core.h: bkt_lds_bytes, bkt_scalar_groups)

The stage fails closed -- a superchunk whose check does not pass falls through to the chunks of 8 and from there to the exact check -- so
a kernel that computes a wrong left-hand side or drops a carry costs speed and leaves every accept bit right; the verifier tests cannot
see it.  Here every comparison is exact:

  wab[j]     one Keccak-f[1600] of seed | j | tag; (0, 0) where status[j] != 0
  c4[j]      the canonical words of the projective coordinates handed in
  lhs[c]     decoded from its limbs, brought to affine: sum_j (a_j + b_j lambda) C_j over the superchunk
  asc[c][i]  sum_j (a_j + b_j lambda) s_ji mod n
  sflag[c]   0 exactly when the expected lhs equals sum_i asc_i B_i
  accept     on a passing superchunk 1 for unflagged proofs and 0 for flagged ones; on a failing one still the launcher's sentinel

Every point has a known discrete logarithm: the bases are B_i = beta_i G, a proof's scalars are one of a pool of 64 rows (32 random ones
and their negatives, so that C and -C both occur), and its commitment is C_j = sum_i s_ji B_i unless a case says otherwise, handed over
with a random Z.  The expected lhs of a superchunk is then ONE scalar multiplication of G, whatever M is, and proofs that share a row put
equal points into one bucket.  The M = 8192 cases take a second each on the slower host build, so they run on all three builds.

Measured: the CPU tier (gcc and clang together, libraries built) 14 s for this module, its slowest test 1.9 s; the gfx950 tests 4 s on an
MI355X, the slowest 1.4 s.  Three one-line arithmetic mutants of k_verify_bucket.hip -- five doublings of B instead of six, `<= 64` in
the suffix scan, the carry dropped from the shuffle tree of k_bkt_scalars -- each fail 22 of the 28 gfx950 tests (the first two on lhs,
the third on asc)."""
import random

import numpy as np
import pytest

import bppp_oracle as O
from prims import build as PB

P, NN, LAM = O.P, O.N, O.LAMBDA
M64 = (1 << 64) - 1
SENTINEL = 0xA5
W = 4
NB_MAX = 65
ZERO_ROW, TOP_ROW = 64, 65          # rows of the pool beside the 64 random ones: every scalar 0, every scalar n - 1
MAX_M = 8192
TAG = int.from_bytes(b"BPPP_RLC", "little")
SEED0 = bytes(32)
SEED1 = bytes((37 * i + 11) & 0xFF for i in range(32))


# ---------------------------------------------------------------- the reference: Keccak-f[1600] over all proofs at once
_RC = [np.uint64(x) for x in O._RC]


def _rol(v, r):
    return v if r % 64 == 0 else (v << np.uint64(r % 64)) | (v >> np.uint64(64 - r % 64))


def keccak_lanes(lanes):
    """O.keccak_f1600 over numpy uint64 columns (lanes[x + 5 y]); pinned to the oracle's own permutation by weights()."""
    A = [[lanes[x + 5 * y] for y in range(5)] for x in range(5)]
    for rnd in range(24):
        Cx = [A[x][0] ^ A[x][1] ^ A[x][2] ^ A[x][3] ^ A[x][4] for x in range(5)]
        D = [Cx[(x - 1) % 5] ^ _rol(Cx[(x + 1) % 5], 1) for x in range(5)]
        A = [[A[x][y] ^ D[x] for y in range(5)] for x in range(5)]
        Bm = [[None] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                Bm[y][(2 * x + 3 * y) % 5] = _rol(A[x][y], O._ROT[x][y])
        A = [[Bm[x][y] ^ (~Bm[(x + 1) % 5][y] & Bm[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        A[0][0] = A[0][0] ^ _RC[rnd]
    return [A[i % 5][i // 5] for i in range(25)]


def weight_halves(seed: bytes, t: int):
    """tests/test_rlc_emul.py: _weight_halves -- the oracle's permutation of seed | index | tag"""
    st = [int.from_bytes(seed[8 * i:8 * i + 8], "little") for i in range(4)] + [t, TAG] + [0] * 19
    out = O.keccak_f1600(st)
    return out[0], out[1]


_WEIGHTS = {}


def weights(seed: bytes, n: int):
    """[(a_j, b_j)] for j < n; every one of them from the oracle for n <= 256, else the ends and 61 spread indices"""
    if (seed, n) not in _WEIGHTS:
        st = [np.zeros(n, np.uint64) for _ in range(25)]
        for i in range(4):
            st[i] += np.uint64(int.from_bytes(seed[8 * i:8 * i + 8], "little"))
        st[4] = np.arange(n, dtype=np.uint64)
        st[5] += np.uint64(TAG)
        out = keccak_lanes(st)
        w = list(zip((int(x) for x in out[0]), (int(x) for x in out[1])))
        for j in range(n) if n <= 256 else {0, 1, n - 2, n - 1, *range(7, n, n // 61)}:
            assert w[j] == weight_halves(seed, j), j
        _WEIGHTS[(seed, n)] = w
    return _WEIGHTS[(seed, n)]


# ---------------------------------------------------------------- bases, the pool of scalar rows, points with known logarithms
_RG = random.Random(0xB0C4E7)
BLOG = [_RG.randrange(1, NN) for _ in range(NB_MAX)]                 # B_i = BLOG[i] G
ROWS = [[_RG.randrange(1, NN) for _ in range(NB_MAX)] for _ in range(32)]
ROWS += [[NN - s for s in r] for r in ROWS] + [[0] * NB_MAX, [NN - 1] * NB_MAX]
_POINTS = {0: None}


def point(log):
    """log G, remembered (and -log G with it)"""
    log %= NN
    if log not in _POINTS:
        p = O.pt_mul(O.G, log)
        _POINTS[log] = p
        _POINTS[NN - log] = O.pt_neg(p)
    return _POINTS[log]


def row_log(k, nb):
    return sum(s * b for s, b in zip(ROWS[k][:nb], BLOG)) % NN


def limbs26(x):
    return [(x >> (26 * i)) & 0x3FFFFFF for i in range(9)] + [x >> 234]


def rep(x, m, rg):
    """limbs of x mod p at magnitude <= m: random limbs of magnitude m - 1 plus the canonical limbs of the rest"""
    if m == 1:
        return limbs26(x % P)
    r = [rg.randint(0, 2 * (m - 1) * 0x3FFFFFF) for _ in range(9)] + [rg.randint(0, 2 * (m - 1) * 0x3FFFFF)]
    v = sum(l << (26 * i) for i, l in enumerate(r))
    return [a + b for a, b in zip(limbs26((x - v) % P), r)]


def words8(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def val26(col):
    return sum(int(l) << (26 * i) for i, l in enumerate(col))


_ARRAYS, _EXP = {}, {}          # by case name: computed once, shared by the builds, never changed


class Case:
    """One call of the entry point.  rows[j]: the proof's scalar row; logs: {j: log} where C_j is NOT sum_i s_ji B_i; given: None (the
    weights come from bkt_prepare over `seed`) or [(a_j, b_j)] (crafted digits: wab and c4 are handed in)."""

    def __init__(self, name, N, M, nb, rows, seed=SEED1, flagged=(), logs=None, given=None):
        assert len(rows) == N and (given is None or len(given) == N)
        self.name, self.N, self.M, self.nb, self.rows, self.seed, self.given = name, N, M, nb, list(rows), seed, given
        self.ns = (N + M - 1) // M
        self.status = [0] * N
        for k, j in enumerate(flagged):
            self.status[j] = (1, 3, -1)[k % 3]
        own = {k: row_log(k, nb) for k in set(self.rows)}
        self.logs = [own[k] for k in self.rows]
        for j, lg in (logs or {}).items():
            self.logs[j] = lg % NN

    # ---- the arrays handed over
    def arrays(self):
        if self.name not in _ARRAYS:
            _ARRAYS[self.name] = self._arrays()
        return _ARRAYS[self.name]

    def _arrays(self):
        rg = random.Random(self.name)
        N, nb = self.N, self.nb
        coords = []
        for j, lg in enumerate(self.logs):
            p = point(lg)
            z = rg.randrange(1, P)
            coords.append((0, z, 0) if p is None else (p[0] * z % P, p[1] * z % P, z))
        acc = np.zeros((30, N), np.uint32)
        for j, (X, Y, Z) in enumerate(coords):
            if j % 5 == 2:      # at the magnitudes ws_ld_pt promises the group law: (5, 2, 2)
                col = rep(X, 5, rg) + rep(Y, 2, rg) + rep(Z, 2, rg)
            else:
                col = limbs26(X) + limbs26(Y) + limbs26(Z)
            acc[:, j] = col
        c4 = np.array([words8(X) + words8(Y) + words8(Z) for X, Y, Z in coords], np.uint32)
        roww = {k: np.array([w for s in ROWS[k][:nb] for w in words8(s)], np.uint32) for k in set(self.rows)}
        fsc = np.ascontiguousarray(np.stack([roww[k] for k in self.rows], axis=1))
        assert fsc.shape == (nb * 8, N)
        return coords, acc, c4, fsc

    # ---- what the oracle says
    def weights(self):
        w = self.given if self.given is not None else weights(self.seed, self.N)
        return [(a, b) if st == 0 or self.given is not None else (0, 0) for (a, b), st in zip(w, self.status)]

    def expected(self):
        if self.name not in _EXP:
            wab = self.weights()
            ws = [(a + b * LAM) % NN for a, b in wab]
            lhs, asc, sflag = [], [], []
            accept = [SENTINEL] * self.N
            for c in range(self.ns):
                js = range(c * self.M, min((c + 1) * self.M, self.N))
                lhs.append(point(sum(ws[j] * self.logs[j] for j in js)))
                A = [sum(ws[j] * ROWS[self.rows[j]][i] for j in js) % NN for i in range(self.nb)]
                asc.append(A)
                ok = lhs[c] == point(sum(a * b for a, b in zip(A, BLOG)))
                sflag.append(0 if ok else 1)
                if ok:
                    for j in js:
                        accept[j] = 1 if self.status[j] == 0 else 0
            _EXP[self.name] = (wab, lhs, asc, sflag, accept)
        return _EXP[self.name]


# ---------------------------------------------------------------- running and comparing
_LIB, _TABLE, _OUT = {}, {}, {}
GENS = None


def lib_of(backend):
    if backend not in _LIB:
        why = PB.unavailable(backend)
        if why:
            pytest.skip(f"{backend} backend skipped: {why}")
        _LIB[backend] = PB.load(backend)
    return _LIB[backend]


def table_of(backend):
    """the fixed-base table of all NB_MAX bases (a call with fewer bases uses its head), built by the backend's own host code"""
    global GENS
    if backend not in _TABLE:
        L = lib_of(backend)
        if GENS is None:
            GENS = b"".join(O.pt_to_xy64(point(b)) for b in BLOG)
        tab = np.zeros(L.prims_bucket_fb_entries(NB_MAX, W) * 64, np.uint8)
        assert L.prims_bucket_fb_build(GENS, NB_MAX, W, tab.ctypes.data) == 0
        _TABLE[backend] = tab
    return _TABLE[backend]


def run(backend, case):
    """every output of one call, as numpy arrays: wab [N][2], c4 [N][24], lhs [30][ns], asc [nb * 8][ns], sflag [ns], accept [N]"""
    key = (backend, case.name)
    if key in _OUT:
        return _OUT[key]
    L, tab = lib_of(backend), table_of(backend)
    coords, acc, c4_in, fsc = case.arrays()
    N, ns, nb = case.N, case.ns, case.nb
    seed = np.frombuffer(case.seed, np.uint64).copy()
    status = np.array(case.status, np.int32)
    given = case.given is not None
    wab = np.array(case.given, np.uint64).reshape(N, 2) if given else np.full((N, 2), 0x5A5A5A5A5A5A5A5A, np.uint64)
    c4 = c4_in.copy() if given else np.full((N, 24), 0x5A5A5A5A, np.uint32)
    lhs = np.full((30, ns), 0x5A5A5A5A, np.uint32)
    asc = np.full((nb * 8, ns), 0x5A5A5A5A, np.uint32)
    sflag, accept = np.zeros(ns, np.uint8), np.zeros(N, np.uint8)
    rc = L.run_bucket(N, case.M, nb, seed.ctypes.data, status.ctypes.data, acc.ctypes.data, fsc.ctypes.data, tab.ctypes.data, W,
                      1 if given else 0, wab.ctypes.data, c4.ctypes.data, lhs.ctypes.data, asc.ctypes.data, sflag.ctypes.data,
                      accept.ctypes.data)
    assert rc == 0, f"{case.name}: run returned {rc}"
    _OUT[key] = (wab, c4, lhs, asc, sflag, accept, c4_in)
    return _OUT[key]


def decode_point(lhs, c):
    X, Y, Z = (val26(lhs[10 * k:10 * k + 10, c]) % P for k in range(3))
    if Z == 0:
        assert X == 0 and Y != 0, "a point at infinity is (0 : y : 0)"
        return None
    zi = pow(Z, -1, P)
    p = (X * zi % P, Y * zi % P)
    assert O.on_curve(p)
    return p


def check(backend, case):
    """every output of the call against the oracle; returns the outputs"""
    wab, c4, lhs, asc, sflag, accept, c4_in = out = run(backend, case)
    e_wab, e_lhs, e_asc, e_sflag, e_accept = case.expected()
    what = f"{case.name} on {backend}"
    got_w = [(int(a), int(b)) for a, b in wab]
    bad = [j for j in range(case.N) if got_w[j] != e_wab[j]]
    assert not bad, f"{what}: wab wrong at proofs {bad[:8]}"
    assert (c4 == c4_in).all(), f"{what}: c4 wrong at proofs {sorted(set(np.nonzero(c4 != c4_in)[0].tolist()))[:8]}"
    for c in range(case.ns):
        assert decode_point(lhs, c) == e_lhs[c], f"{what}: lhs of superchunk {c}"
        got = [sum(int(asc[8 * i + k, c]) << (32 * k) for k in range(8)) for i in range(case.nb)]
        bad = [i for i in range(case.nb) if got[i] != e_asc[c][i]]
        assert not bad, f"{what}: asc of superchunk {c} wrong at bases {bad[:8]}"
    assert sflag.tolist() == e_sflag, f"{what}: sflag {sflag.tolist()}, expected {e_sflag}"
    bad = [j for j in range(case.N) if int(accept[j]) != e_accept[j]]
    assert not bad, f"{what}: accept wrong at proofs {bad[:8]}: {[int(accept[j]) for j in bad[:8]]}"
    return out


def pool_rows(rg, n):
    """n rows of the pool of 64: reuse is wanted (equal points in one bucket, C and -C)"""
    return [rg.randrange(64) for _ in range(n)]


BACKEND_PARAMS = ["gcc", "clang", pytest.param("gfx950", marks=pytest.mark.gpu)]


@pytest.fixture(scope="module", params=BACKEND_PARAMS)
def backend(request):
    return request.param


# ---------------------------------------------------------------- the launcher's own pieces
def test_launch_geometry(backend):
    """bkt_lds_bytes / bkt_scalar_groups, which launch_bucket_stage and the launcher share: per wavefront 256 cursors, 256 bucket starts and
    2 M 16-bit item numbers, then 8 window sums of 30 words; one workgroup per 16 bases.  The largest superchunk fits the 160 KB of LDS."""
    L = lib_of(backend)
    for M in (1, 64, 72, 256, 4096, MAX_M):
        for nb in (1, 16, 17, 49, 65, 769):
            out = (PB.C.c_uint64 * 2)()
            L.prims_bucket_geometry(M, nb, out)
            assert out[0] == 4 * (256 * 4 + 256 * 4 + 2 * M * 2) + 8 * 30 * 4 and out[0] <= 160 * 1024
            assert out[1] == -(-nb // 16)


def test_fixed_base_table_entries(backend):
    """the table the check reads: entry d - 1 of window w of base i is d 2^(4 w) B_i, affine, in packed canonical words"""
    tab = table_of(backend).view(np.uint32).reshape(NB_MAX, 64, 15, 16)
    rg = random.Random(3)
    for i, w, d in [(0, 0, 1), (0, 63, 15), (NB_MAX - 1, 63, 15), (2, 1, 8)] + [(rg.randrange(NB_MAX), rg.randrange(64), rg.randrange(1, 16))
                                                                                 for _ in range(12)]:
        e = point(d * BLOG[i] << (4 * w))
        assert tab[i, w, d - 1].tolist() == words8(e[0]) + words8(e[1]), (i, w, d)


def test_arguments_out_of_range_are_refused(backend):
    """nothing runs for a superchunk size the LDS layout cannot hold, no proofs, no bases or another table width"""
    L, tab = lib_of(backend), table_of(backend)
    z = np.zeros(64 * 30, np.uint32)
    for N, M, nb, w in ((0, 64, 3, W), (4, 0, 3, W), (4, MAX_M + 1, 3, W), (4, 64, 0, W), (4, 64, 3, 8)):
        rc = L.run_bucket(N, M, nb, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, tab.ctypes.data, w, 0, z.ctypes.data,
                          z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data)
        assert rc != 0 and not z.any(), (N, M, nb, w)


# ---------------------------------------------------------------- layout: through bkt_prepare
LAYOUTS = ((64, 1), (64, 64), (64, 65), (72, 143), (256, 700), (MAX_M, MAX_M + 1))


def layout_case(M, N, seed):
    rg = random.Random(f"layout {M} {N}")
    flagged = sorted({0, M - 1, N - 1} & set(range(N)))          # proof 0, a superchunk's last proof, the batch's last proof
    return Case(f"layout M={M} N={N} seed={seed[:2].hex()}", N, M, 3, pool_rows(rg, N), seed=seed, flagged=flagged)


@pytest.mark.parametrize("seed", (SEED0, SEED1), ids=("seed0", "seed1"))
@pytest.mark.parametrize("M,N", LAYOUTS)
def test_layouts(backend, M, N, seed):
    """Superchunk sizes and batch lengths around the wavefront, a size that is neither a power of two nor a multiple of 64, the LDS
    maximum, partial last superchunks down to one proof; flagged proofs at the ends.  Every proof is valid, so every superchunk passes."""
    case = layout_case(M, N, seed)
    _, _, _, _, sflag, accept, _ = check(backend, case)
    assert not sflag.any()
    assert accept.tolist() == [1 if s == 0 else 0 for s in case.status]


# ---------------------------------------------------------------- crafted digits
def digit_cases(M):
    N = M + 5                                        # a second superchunk of 5 proofs under the same digits
    rg = random.Random(f"digits {M}")
    rows = pool_rows(rg, N)
    out = []

    def add(name, given, rows=rows, **kw):
        out.append(Case(f"digits M={M}: {name}", N, M, 3, rows, given=given, **kw))
    add("every weight zero", [(0, 0)] * N)
    add("every half-weight 2^64 - 1", [(M64, M64)] * N)                        # all 2 M items in bucket 255 of every window
    for d in (64, 128, 192, 1, 63):                                            # lane 0's buckets beside the excluded digit 0; lanes 1, 63
        add(f"every digit {d}", [(d * 0x0101010101010101,) * 2] * N)
    for w in range(8):                                                         # wave-to-window mapping, the Horner doublings
        add(f"only window {w}", [(rg.randrange(1, 256) << (8 * w), rg.randrange(1, 256) << (8 * w)) for _ in range(N)])
    add("a = b", [(a, a) for a in (rg.getrandbits(64) for _ in range(N))])    # C and phi(C) in one bucket
    pr = [rg.randrange(32) for _ in range((N + 1) // 2)]
    pw = [(rg.getrandbits(64), rg.getrandbits(64)) for _ in pr]
    add("pairs C, -C", [pw[j // 2] for j in range(N)], rows=[pr[j // 2] + 32 * (j % 2) for j in range(N)])
    idrows = list(rows)
    idrows[M // 3] = ZERO_ROW                                                  # C = the identity, handed over as (0 : y : 0)
    add("one C is the identity", [(rg.getrandbits(64), rg.getrandbits(64)) for _ in range(N)], rows=idrows)
    for j0, ab in ((M // 2, (rg.getrandbits(64), 0)), (M - 1, (0, rg.getrandbits(64))), (0, (0x80 << 56, 0))):
        add(f"proof {j0} alone", [ab if j == j0 else (0, 0) for j in range(N)])
    return out


@pytest.mark.parametrize("M", (64, 256))
def test_crafted_digits(backend, M):
    """Hand-made half-weights through the sort, the lane-owned buckets, the suffix scan and Horner; each compared on lhs (and on all else)."""
    cases = digit_cases(M)
    assert len(cases) == 21
    for case in cases:
        _, _, lhs, _, sflag, _, _ = check(backend, case)
        assert not sflag.any(), case.name                # the scalars are the rows' own, so both sides of every check agree
        if "weight zero" in case.name:
            assert decode_point(lhs, 0) is None and decode_point(lhs, 1) is None
        if "pairs" in case.name:
            assert decode_point(lhs, 0) is None         # (the second superchunk ends on a C without its -C)


# ---------------------------------------------------------------- the combined scalars
def scalar_cases():
    out = []
    for nb in (1, 16, 17, 49, 65):                   # around BPPP_BKT_SCALAR_GROUP and the 64 lanes of fb_group_sum<64>
        rg = random.Random(f"scalars {nb}")
        out.append(Case(f"scalars nb={nb}", 64 + 7, 64, nb, pool_rows(rg, 71), flagged=(5,)))
    # the largest unreduced sum: 8192 terms of (2^64 - 1) (n - 1) per half-weight
    out.append(Case("scalars largest sum", MAX_M, MAX_M, 3, [TOP_ROW] * MAX_M, given=[(M64, M64)] * MAX_M))
    out.append(Case("scalars all zero", 64, 64, 3, [ZERO_ROW] * 64, logs={j: 1 + j % 7 for j in range(64)}))
    rg = random.Random("scalars 200")
    out.append(Case("scalars M=200", 2 * 200 + 13, 200, 3, pool_rows(rg, 413)))     # fewer proofs than threads in the last round
    return out


@pytest.mark.parametrize("k", range(8), ids=lambda k: ("nb1", "nb16", "nb17", "nb49", "nb65", "largest", "zero", "M200")[k])
def test_combined_scalars(backend, k):
    case = scalar_cases()[k]
    _, _, _, _, sflag, _, _ = check(backend, case)
    if case.name == "scalars all zero":
        assert sflag.all()          # the right-hand side is the identity, the left-hand side is not
    else:
        assert not sflag.any()


# ---------------------------------------------------------------- the check and its verdict bytes
CHECK_M, CHECK_N = 64, 2 * 64 + 1                    # two full superchunks and one of a single proof
CHECK_AT = (64, 127, 30, 128)                        # first and last proof of a superchunk, a middle one, the lone proof of the partial one


def check_case(nb, what, j=None):
    rg = random.Random(f"check {nb}")
    rows = pool_rows(rg, CHECK_N)
    if what == "valid":
        return Case(f"check nb={nb}: all valid", CHECK_N, CHECK_M, nb, rows)
    other = row_log((rows[j] + 1) % 64, nb)           # another pool point
    if what == "bad":
        return Case(f"check nb={nb}: wrong C at {j}", CHECK_N, CHECK_M, nb, rows, logs={j: other})
    return Case(f"check nb={nb}: flagged wrong C at {j}", CHECK_N, CHECK_M, nb, rows, logs={j: other}, flagged=(j,))


@pytest.mark.parametrize("nb", (3, 65))
def test_check_verdicts(backend, nb):
    """C_j = sum_i s_ji B_i passes everywhere; one foreign C_j flags exactly its superchunk and leaves that superchunk's accept bytes
    untouched; the same C_j on a flagged proof has weight zero and fails nothing."""
    _, _, _, _, sflag, accept, _ = check(backend, check_case(nb, "valid"))
    assert not sflag.any() and (accept == 1).all()
    for j in CHECK_AT:
        _, _, _, _, sflag, accept, _ = check(backend, check_case(nb, "bad", j))
        c = j // CHECK_M
        assert sflag.tolist() == [1 if k == c else 0 for k in range(3)], j
        assert [int(a) for a in accept] == [SENTINEL if t // CHECK_M == c else 1 for t in range(CHECK_N)], j
        _, _, _, _, sflag, accept, _ = check(backend, check_case(nb, "flagged", j))
        assert not sflag.any(), j
        assert [int(a) for a in accept] == [0 if t == j else 1 for t in range(CHECK_N)], j


# ---------------------------------------------------------------- one answer on every build
def test_same_bits_everywhere(backend):
    """gcc, clang and gfx950 give identical wab, c4 and asc words (lhs is a projective class: compared as a point above)."""
    others = [b for b in ("gcc", "clang") if b != backend and PB.unavailable(b) is None]
    if not others:
        pytest.skip("no second build to compare with")
    cases = [layout_case(M, N, SEED1) for M, N in LAYOUTS[:5]] + digit_cases(64) + scalar_cases() + [check_case(65, "bad", 127)]
    for case in cases:
        mine = run(backend, case)
        for other in others:
            theirs = run(other, case)
            for k, name in ((0, "wab"), (1, "c4"), (3, "asc")):
                assert (mine[k] == theirs[k]).all(), f"{case.name}: {name} differs between {backend} and {other}"
