"""Conformance of the field, scalar and group primitives (bp_pp_amd/csrc: field.h, modinv.h, point.h, straus_core.h, draw_core.h,
verify_core.h) at constructed edge inputs, against big integers, on three builds of one case dispatcher (tests/prims/prims_core.h):

  gcc     g++ host build: the code path of the tests/emul emulation
  clang   ROCm clang++ host build: field.h's __builtin_addc / __builtin_subc carry chains
  gfx950  the hipcc --offload-arch=gfx950 -O3 build, one record per lane (marked gpu): the code the kernels run, with the
          v_mad_u64_u32 / v_addc asm of mad_c / add_c, opaque_u32 and the alignbit rotate

Operands enter as raw limb vectors at the bounds of each function's contract (magnitude m: limbs <= 2m (2^26 - 1), top limb
<= 2m (2^22 - 1)); the host builds declare every operand's magnitude, so field.h's FE_CHECK asserts guard that contract.  Every
record is checked three ways, all exact: its value against the big-integer reference, its raw output words against what the
function promises (magnitude-1 limbs after a product, canonical after fe_normalize, below n for every scalar), and its raw words
against the other builds (identical bits, not merely congruent).  On the device the record set runs shuffled (wavefronts mix op
codes and byte offsets) and sorted by op code (uniform wavefronts); both runs must agree word for word.

Three families go past single calls.  `accum`: programs of up to 12 steps (ptj_dbl, ptj_madd / ptz_madd with a skip bit) over the
incomplete Jacobian and XYZZ accumulators and their conversion, from the empty accumulator or raw limbs at the magnitude bounds,
with acc = q and acc = -q at the first, a middle and the last step: where no exceptional addition occurred the result is the
big-integer sum, where one did Z (ZZ) is 0 mod p after that step and every later one.  `recode`: glv_recode5, glv_window_digits and
glv_digit_of for glv_words<1 .. 5>: the 26 digits rebuild the signed half-scalar of glv_model and stay within the 16 table entries.
`table`: affine_table_one for every number of doublings split_begin yields, entry by entry, with the beta-frame twin.

The variable-base SUMS have records and kernels of their own (prims_core.h: SumForm): straus_affine, straus_affine_fast +
straus_affine_complete, straus_affine_complete and straus_split_lane on one lane (all builds), straus_affine_g4<M, G> and
straus_affine_split<M, G, PARTS> on their real lane groups (device), over tables built by affine_tables_build / affine_table_one.
Every sum is compared with sum_i k_i P_i of the oracle, for equal, opposite and identity points too, so a fallback that returned a
wrong point fails here; the fast forms' flag is compared with a group-element model of the same lane.

The TRANSCRIPT primitives (merlin.h: Keccak-f, the STROBE steps, the merlin operations; app_point; for_each_position_group) are a third
family with records, entry points and launch layouts of their own (prims_core.h: TrStep), tested by tests/test_prims_transcript.py."""
import math
import random
import struct

import numpy as np
import pytest

import bppp_oracle as O
import chacha_ref
from prims import build as PB

P, N, LAM, BETA = O.P, O.N, O.LAMBDA, O.BETA
ND = 2**256 - N
M26, M22 = (1 << 26) - 1, (1 << 22) - 1
IN_W, OUT_W = 176, 200
SUM_IN_W, SUM_OUT_W = 128, 80

# op codes: prims_core.h enum Op
FE_MUL, FE_SQR, FE_MUL2_ADD, FE_MUL_SMALL, FE_ADD, FE_SUB_M, FE_NEG_M, FE_NORMALIZE = range(1, 9)
FE_IS_ZERO, FE_IS_ODD, FE_EQ, FE_TO_W8, FE_FROM_W8, FE_INV, FE_INV_FERMAT, FE_SQRT, FE_BATCH_INV = range(9, 18)
SC_ADD, SC_SUB, SC_NEG, SC_MUL, SC_SQR, SC_REDUCE512, DRAW_REDUCE512, SC_INV, SC_INV_FERMAT = range(32, 41)
BE32_TO_LIMBS, FE_FROM_BE, SC_FROM_BE, SEC1_DECOMPRESS, LIMBS_TO_BE32 = range(48, 53)
PT_ADD, PT_DBL, PT_MADD_NONID, PT_MADD = range(64, 68)
GLV, DRAW_SCALAR = 80, 81
ACCUM, RECODE, TABLE = 96, 97, 98

FAMILIES = ("fp_products", "fp_linear", "fp_normalize", "fn", "fn_wrap", "inversion", "bytes_sec1", "group", "glv", "draw",
            "accum", "recode", "table")

# ---------------------------------------------------------------- limb vectors
P_LIMBS = [0x3FFFC2F, 0x3FFFFBF] + [M26] * 7 + [M22]                 # p itself, 26-bit limbs
ZV = [2 * v for v in P_LIMBS]                                          # the vector fe_sub_m adds per unit: 2p, magnitude exactly 1


def val(v):
    return sum(int(x) << (26 * i) for i, x in enumerate(v))


def limbs(x):   # canonical split of 0 <= x < 2^256 (magnitude 1)
    assert 0 <= x < 1 << 256
    return [(x >> (26 * i)) & M26 for i in range(9)] + [x >> 234]


def vadd(a, b):
    return [x + y for x, y in zip(a, b)]


def noncanon(x, j):   # x mod p plus j copies of ZV: value x, magnitude 1 + j
    v = limbs(x % P)
    for _ in range(j):
        v = vadd(v, ZV)
    return v


def maxv(m):   # every limb at the bound of magnitude m
    return [2 * m * M26] * 9 + [2 * m * M22]


def rnd_limbs(m, rg):
    return [rg.randint(0, 2 * m * M26) for _ in range(9)] + [rg.randint(0, 2 * m * M22)]


def rep(x, m, rg):   # a random representation of x mod p with magnitude <= m
    r = rnd_limbs(m - 1, rg) if m > 1 else [0] * 10
    return vadd(limbs((x - val(r)) % P), r)


def mag_ok(v, m):
    return all(int(v[i]) <= 2 * m * M26 for i in range(9)) and int(v[9]) <= 2 * m * M22


def canonical(v):
    return all(int(v[i]) <= M26 for i in range(9)) and int(v[9]) <= M22 and val(v) < P


def reduced(v):
    """What fe_reduce_cols promises (its comments): limbs 0-2 and 4-8 below 2^26, limb 3 below 2^26 + 2^8 ("f < 2^8"), limb 9
    below 2^22 -- in particular magnitude 1."""
    return all(int(v[i]) <= M26 for i in (0, 1, 2, 4, 5, 6, 7, 8)) and int(v[3]) < (1 << 26) + (1 << 8) and int(v[9]) <= M22


def w8(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def wval(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


def fold_wrap(t):
    """Python model of the three folds by 2^256 - n (sc_reduce512 / draw_reduce512): True when the last fold carries past 2^256
    (the d[8] branch)."""
    a = (t % 2**256) + (t >> 256) * ND
    b = (a % 2**256) + (a >> 256) * ND
    d = (b % 2**256) + (b >> 256) * ND
    return d >= 2**256


def wrap_inputs(count, rg):
    """Values t < n^2 whose reduction takes the last wrap (the construction of the issue's note): pick a = t - floor(t / 2^256) ND
    with a_hi = H = floor(2^256 / ND) - delta and a_lo in the window that makes the second fold cross 2^257 - ND, then solve for t."""
    out = []
    for dh in range(64):
        H = 2**256 // ND - dh
        base = H * ND
        lo_, hi_ = max(2**257 - ND - base, 0), min(2**257 - base, 2**256)
        for _ in range(40 if lo_ < hi_ else 0):
            a = H * 2**256 + rg.randrange(lo_, hi_)
            T = a // ND
            t = T * 2**256 + (a - T * ND)
            if T < 2**256 and t < N * N:
                out.append(t)
        if len(out) >= count:
            break
    return out[:count]


def wrap_products(ts):
    """x, y < n with x y = a t' near each t that still takes the wrap: x = s + u, y = s - u with s just above sqrt(t)."""
    pairs = []
    for t in ts:
        for ds in range(4000):
            s = math.isqrt(t) + 1 + ds
            u0 = math.isqrt(s * s - t)
            hit = [(s + u, s - u) for u in range(max(u0 - 2, 0), u0 + 3) if s + u < N and fold_wrap((s + u) * (s - u))]
            if hit:
                pairs.append(hit[0])
                break
    return pairs


# ---------------------------------------------------------------- the record set
class Cases:
    def __init__(self):
        self.recs, self.meta = [], []
        self.bytes = bytearray(64)      # offsets are taken mod 16 against a 64-byte aligned buffer (both host and device)
        self.same_probe = []            # (record, record): two accumulator programs whose probed raw limbs must be identical

    def add(self, family, op, words=(), mags=(), p2=0, p3=0, check=None, desc=""):
        r = [0] * IN_W
        r[0], r[1], r[2], r[3] = op, sum(m << (8 * k) for k, m in enumerate(mags)), p2, p3
        words = [int(w) for w in words]
        assert len(words) <= IN_W - 4 and all(0 <= w < 1 << 32 for w in words), desc
        r[4:4 + len(words)] = words
        self.recs.append(r)
        self.meta.append((family, check, desc))

    def put_bytes(self, data, mod16):
        while len(self.bytes) % 16 != mod16:
            self.bytes.append(0xEE)
        off = len(self.bytes)
        self.bytes += data
        self.bytes += b"\xEE" * 3
        return off


def _fe_products(C, rg):
    F = "fp_products"

    def prod_check(expect):
        def chk(o):
            r = o[:10]
            assert val(r) % P == expect % P, "value"
            assert reduced(r), "fe_reduce_cols bound"
        return chk

    mags = (1, 2, 4, 8)
    for ma in mags:
        for mb in mags:
            ops = [(maxv(ma), maxv(mb))] + [(rnd_limbs(ma, rg), rnd_limbs(mb, rg)) for _ in range(3)] + \
                  [(rep(P - 1, ma, rg), maxv(mb)), (noncanon(rg.randrange(P), ma - 1), noncanon(P - 1, mb - 1))]
            for a, b in ops:
                C.add(F, FE_MUL, a + b, (ma, mb), check=prod_check(val(a) * val(b)), desc=f"fe_mul {ma}x{mb}")
        for a in [maxv(ma)] + [rnd_limbs(ma, rg) for _ in range(4)] + [noncanon(P - 1, ma - 1), limbs(2**256 - 1) if ma == 1 else maxv(ma)]:
            C.add(F, FE_SQR, a, (ma,), check=prod_check(val(a) ** 2), desc=f"fe_sqr {ma}")
    for x in (0, 1, P - 1, 2**256 - 1, 2**255):
        a = limbs(x)
        C.add(F, FE_MUL, a + a, (1, 1), check=prod_check(x * x), desc="fe_mul canonical-limb edges")
    zero = [0] * 10
    splits = [((8, 8), (0, 8)), ((4, 8), (4, 8)), ((1, 8), (7, 8)), ((8, 1), (8, 7)), ((2, 8), (6, 8)), ((8, 8), (0, 0))]
    for (ma, mb), (mc, md) in splits:
        for kind in ("max", "rnd", "rnd"):
            g = (lambda m: maxv(m) if m else zero) if kind == "max" else (lambda m: rnd_limbs(m, rg) if m else zero)
            a, b, c, d = g(ma), g(mb), g(mc), g(md)
            C.add(F, FE_MUL2_ADD, a + b + c + d, (ma, mb, mc, md), check=prod_check(val(a) * val(b) + val(c) * val(d)),
                  desc=f"fe_mul2_add {ma}*{mb}+{mc}*{md} {kind}")

    def small_check(expect):
        def chk(o):
            r = o[:10]
            assert val(r) % P == expect % P, "value"
            assert mag_ok(r, 1), "magnitude 1"
            assert all(int(r[i]) <= M26 for i in (0, 1, 3, 4, 5, 6, 7, 8)) and int(r[9]) <= M22, "limbs other than 2 are 26/22-bit"
        return chk

    for k in (0, 1, 2, 3, 8, 21, 32):
        for a in [maxv(8), noncanon(P - 1, 7)] + [rnd_limbs(8, rg) for _ in range(3)]:
            C.add(F, FE_MUL_SMALL, a, (8,), p2=k, check=small_check(val(a) * k), desc=f"fe_mul_small k={k}")


def _fe_linear(C, rg):
    F = "fp_linear"

    def exact(expect_limbs, expect_mod, m):
        def chk(o):
            r = [int(v) for v in o[:10]]
            assert r == expect_limbs, "limbs"
            assert val(r) % P == expect_mod % P, "value"
            assert mag_ok(r, m), "magnitude"
        return chk

    for ma, mb in ((8, 8), (1, 15), (15, 1), (4, 12), (1, 1)):
        for a, b in [(maxv(ma), maxv(mb)), (rnd_limbs(ma, rg), rnd_limbs(mb, rg)), (rep(P - 1, ma, rg), rep(P - 1, mb, rg))]:
            C.add(F, FE_ADD, a + b, (ma, mb), check=exact(vadd(a, b), val(a) + val(b), ma + mb), desc=f"fe_add {ma}+{mb}")
    for M in range(1, 7):
        k = 2 * (M + 1)
        ma = 15 - M
        for a, b in [(maxv(ma), maxv(M)), (maxv(ma), [0] * 10), ([0] * 10, maxv(M)), (rnd_limbs(ma, rg), maxv(M)),
                     (rnd_limbs(ma, rg), rnd_limbs(M, rg)), (noncanon(5, ma - 1), noncanon(P - 1, M - 1))]:
            e = [a[i] + k * P_LIMBS[i] - b[i] for i in range(10)]
            C.add(F, FE_SUB_M, a + b, (ma, M), p2=M, check=exact(e, val(a) - val(b), ma + M + 1), desc=f"fe_sub_m<{M}>")
    for M in (1, 3):
        k = 2 * (M + 1)
        for a in (maxv(M), [0] * 10, rnd_limbs(M, rg), noncanon(1, M - 1)):
            e = [k * P_LIMBS[i] - a[i] for i in range(10)]
            C.add(F, FE_NEG_M, a, (M,), p2=M, check=exact(e, -val(a), M + 1), desc=f"fe_neg_m<{M}>")


def _fe_normalize(C, rg):
    F = "fp_normalize"

    def norm_check(x):
        def chk(o):
            r = o[:10]
            assert canonical(r), "canonical"
            assert val(r) == x % P, "value"
        return chk

    for m in range(1, 17):
        for a in [maxv(m), noncanon(P - 1, m - 1), noncanon(0, m - 1), noncanon(rg.randrange(P), m - 1)] + \
                 [rnd_limbs(m, rg) for _ in range(6)]:
            C.add(F, FE_NORMALIZE, a, (m,), check=norm_check(val(a)), desc=f"fe_normalize mag {m}")
    for x in list(range(P - 2, P + 513)) + list(range(2**256 - 512, 2**256)):
        C.add(F, FE_NORMALIZE, limbs(x), (1,), check=norm_check(x), desc=f"fe_normalize {x - P:+d} from p")

    def flag(expect):
        def chk(o):
            assert int(o[0]) == int(expect), "flag"
        return chk

    # non-canonical zeros k p (magnitude ceil(k / 2)) and their neighbours
    for k in range(0, 33):
        z = [k * v for v in P_LIMBS]
        m = max(1, (k + 1) // 2)
        C.add(F, FE_IS_ZERO, z, (m,), check=flag(True), desc=f"fe_is_zero {k}p")
        C.add(F, FE_IS_ODD, z, (m,), check=flag(False), desc=f"fe_is_odd {k}p")
        zp1 = vadd(z, limbs(1))
        C.add(F, FE_IS_ZERO, zp1, (m,), check=flag(False), desc=f"fe_is_zero {k}p+1")
        C.add(F, FE_IS_ODD, zp1, (m,), check=flag(True), desc=f"fe_is_odd {k}p+1")
        if k <= 14:             # fe_eq: magnitudes <= 8
            x = rg.randrange(P)
            mx = max(1, (k + 1) // 2)
            C.add(F, FE_EQ, z + [0] * 10, (mx, 0), check=flag(True), desc=f"fe_eq {k}p 0")
            C.add(F, FE_EQ, vadd(z, limbs(x)) + limbs(x), (mx + 1, 1), check=flag(True), desc=f"fe_eq {k}p+x x")
            C.add(F, FE_EQ, vadd(z, limbs(x)) + limbs((x + 1) % P), (mx + 1, 1), check=flag(False), desc=f"fe_eq {k}p+x x+1")
    for x in (1, 2, P - 1, P - 2, rg.randrange(P)):
        for m in (1, 8, 16):
            a = noncanon(x, m - 1)
            C.add(F, FE_IS_ZERO, a, (m,), check=flag(False), desc="fe_is_zero nonzero")
            C.add(F, FE_IS_ODD, a, (m,), check=flag(x & 1), desc="fe_is_odd")
    for x in (P - 1, P, P + 1, 2**256 - 1):   # magnitude-1 limbs of values at and above p
        C.add(F, FE_IS_ODD, limbs(x), (1,), check=flag((x % P) & 1), desc="fe_is_odd >= p")

    def to_w8_check(x):
        def chk(o):
            assert [int(w) for w in o[:8]] == w8(x % P), "fe_to_w8"
            assert [int(v) for v in o[8:18]] == limbs(x % P), "fe_from_w8 round trip"
        return chk

    for m in range(1, 17):
        for a in (maxv(m), rnd_limbs(m, rg)):
            C.add(F, FE_TO_W8, a, (m,), check=to_w8_check(val(a)), desc=f"fe_to_w8 mag {m}")
    for x in (0, 1, P - 1, P, P + 1, 2**256 - 1, rg.randrange(P)):
        C.add(F, FE_TO_W8, limbs(x), (1,), check=to_w8_check(x), desc="fe_to_w8 edge")

    def from_w8_check(x):
        def chk(o):
            assert [int(v) for v in o[:10]] == limbs(x), "fe_from_w8"
            assert [int(w) for w in o[10:18]] == w8(x % P), "fe_to_w8 round trip"
        return chk

    for x in (0, 1, P - 1, P, P + 1, 2**256 - 1, 2**255, 2**234 - 1, 2**234) + tuple(rg.getrandbits(256) for _ in range(8)):
        C.add(F, FE_FROM_W8, w8(x), check=from_w8_check(x), desc="fe_from_w8")


SC_EDGES = [0, 1, 2, N - 1, N - 2, (N - 1) // 2, (N + 1) // 2, 2**255, ND, 2**128 - 1, 2**128 + 1]


def _sc_check(expect):
    def chk(o):
        r = wval(o[:8])
        assert r < N, "below n"
        assert r == expect % N, "value"
    return chk


def _fn(C, rg):
    F = "fn"
    vals = SC_EDGES + [rg.randrange(N) for _ in range(6)]
    for a in vals:
        for b in vals:
            C.add(F, SC_ADD, w8(a) + w8(b), check=_sc_check(a + b), desc="sc_add")
            C.add(F, SC_SUB, w8(a) + w8(b), check=_sc_check(a - b), desc="sc_sub")
            C.add(F, SC_MUL, w8(a) + w8(b), check=_sc_check(a * b), desc="sc_mul")
        C.add(F, SC_NEG, w8(a), check=_sc_check(-a), desc="sc_neg")
        C.add(F, SC_SQR, w8(a), check=_sc_check(a * a), desc="sc_sqr")
    for target in (N - 1, N, N + 1, 2**256 - 1, 2**256, 2**256 + 1, 2 * N - 2):
        for _ in range(4):
            a = rg.randrange(max(0, target - N + 1), min(N, target + 1))
            b = target - a
            assert 0 <= a < N and 0 <= b < N
            C.add(F, SC_ADD, w8(a) + w8(b), check=_sc_check(target), desc=f"sc_add sum {target - N:+d} from n")


def _fn_wrap(C, rg):
    F = "fn_wrap"
    pair = (0xc973e8ecba391009757a0ddaadba25fadc0401328666e89ba35abc67d84448bd,
            0xc973e8ecba391009757a0ddaadba25f6cf60653fa12ee0fef57c526b0d1c7b2d)
    ts = wrap_inputs(24, rg)
    pairs = [pair] + wrap_products(ts[:20])
    assert len(ts) == 24 and len(pairs) == 21
    for x, y in pairs:
        assert x < N and y < N and fold_wrap(x * y), "constructed product takes the last wrap"
        C.add(F, SC_MUL, w8(x) + w8(y), check=_sc_check(x * y), desc="sc_mul last wrap")
        C.add(F, SC_MUL, w8(y) + w8(x), check=_sc_check(x * y), desc="sc_mul last wrap (swapped)")
    for t in ts:
        assert fold_wrap(t), "constructed input takes the last wrap"
        C.add(F, SC_REDUCE512, w8(t % 2**256) + w8(t >> 256), check=_sc_check(t), desc="sc_reduce512 last wrap")
        C.add(F, DRAW_REDUCE512, w8(t % 2**256) + w8(t >> 256), check=_sc_check(t), desc="draw_reduce512 last wrap")
    C.add(F, SC_MUL, w8(N - 1) + w8(N - 1), check=_sc_check((N - 1) ** 2), desc="sc_mul (n-1)^2")
    C.add(F, SC_SQR, w8(N - 1), check=_sc_check((N - 1) ** 2), desc="sc_sqr (n-1)^2")
    ones = [2**256 - 1, 2**255 - 1, 2**224 - 1, 2**160 - 1, 2**128 - 1, 2**96 - 1, 2**32 - 1]
    for a in ones:
        for b in ones:
            t = a * b
            C.add(F, SC_REDUCE512, w8(t % 2**256) + w8(t >> 256), check=_sc_check(t), desc="sc_reduce512 all-ones words")
            if a < N and b < N:
                C.add(F, SC_MUL, w8(a) + w8(b), check=_sc_check(t), desc="sc_mul all-ones words")
    # draw_reduce512 takes any 512-bit value; its d[8] is set by values above n^2 too
    big = [0, 2**512 - 1, 2**511, N * N, N * N - 1]
    for k in (1, 2, 3, 2**128, (2**512 - 1) // N, rg.getrandbits(256), rg.getrandbits(255)):
        big += [k * N - 1, k * N, k * N + 1]
    for dh in range(0, 64, 4):       # the wrap construction without the t < n^2 bound
        H = 2**256 // ND - dh
        lo_, hi_ = max(2**257 - ND - H * ND, 0), min(2**257 - H * ND, 2**256)
        if lo_ < hi_:
            a = H * 2**256 + rg.randrange(lo_, hi_)
            T = a // ND
            t = T * 2**256 + (a - T * ND)
            if T < 2**256:
                assert fold_wrap(t)
                big.append(t)
    for t in big + [rg.getrandbits(512) for _ in range(8)]:
        t %= 2**512
        C.add(F, DRAW_REDUCE512, w8(t % 2**256) + w8(t >> 256), check=_sc_check(t), desc="draw_reduce512")
        C.add(F, SC_REDUCE512, w8(t % 2**256) + w8(t >> 256), check=_sc_check(t), desc="sc_reduce512")


def _inversion(C, rg):
    F = "inversion"

    def fe_inv_check(x, canon):
        def chk(o):
            r = o[:10]
            assert val(r) % P == (pow(x, -1, P) if x % P else 0), "value"
            assert canonical(r) if canon else reduced(r), "bound"
        return chk

    fvals = [0, 1, P - 1, P - 2, (P + 1) // 2] + [2**k for k in (1, 2, 25, 26, 31, 32, 64, 128, 233, 234, 255)] + \
            [rg.randrange(P) for _ in range(6)]
    for x in fvals:
        C.add(F, FE_INV, limbs(x), (1,), check=fe_inv_check(x, True), desc="fe_inv")
        C.add(F, FE_INV_FERMAT, limbs(x), (1,), check=fe_inv_check(x, False), desc="fe_inv_fermat")
    for m in (2, 8):
        for x in (0, 1, P - 1, rg.randrange(P)):
            C.add(F, FE_INV, noncanon(x, m - 1), (m,), check=fe_inv_check(x, True), desc=f"fe_inv mag {m}")
            C.add(F, FE_INV_FERMAT, rep(x, m, rg), (m,), check=fe_inv_check(x, False), desc=f"fe_inv_fermat mag {m}")
        C.add(F, FE_INV, maxv(m), (m,), check=fe_inv_check(val(maxv(m)), True), desc="fe_inv all-max")
    C.add(F, FE_INV, maxv(16), (16,), check=fe_inv_check(val(maxv(16)), True), desc="fe_inv mag 16")
    svals = [0, 1, N - 1, N - 2, (N + 1) // 2] + [2**k for k in (1, 32, 128, 129, 255)] + [rg.randrange(N) for _ in range(6)]
    for x in svals:
        e = pow(x, -1, N) if x else 0
        C.add(F, SC_INV, w8(x), check=_sc_check(e), desc="sc_inv")
        C.add(F, SC_INV_FERMAT, w8(x), check=_sc_check(e), desc="sc_inv_fermat")

    def sqrt_check(x):
        def chk(o):
            r = o[:10]
            assert val(r) % P == pow(x % P, (P + 1) // 4, P), "value"
            assert reduced(r), "fe_reduce_cols bound"
        return chk

    residues = [0, 1, 4, 7 * 7, P - 4] + [rg.randrange(P) ** 2 % P for _ in range(6)]
    nonres = [P - 1, 7]
    while len(nonres) < 8:
        x = rg.randrange(P)
        if pow(x, (P - 1) // 2, P) == P - 1:
            nonres.append(x)
    for i, x in enumerate(residues + nonres):
        m = (1, 2, 8)[i % 3]
        C.add(F, FE_SQRT, rep(x, m, rg), (m,), check=sqrt_check(x), desc="fe_sqrt_candidate")
    # fe_batch_inv_lane<G>: zeros (canonical and p, 2p limbs) at the first, middle and last positions, N not a multiple of G
    for G, ns in ((2, (5, 9)), (4, (7, 13)), (8, (13, 21)), (16, (17, 37))):
        for n in ns:
            xs = [rg.randrange(1, P) for _ in range(n)]
            vecs = [rep(x, 2, rg) for x in xs]
            for t, z in ((0, [0] * 10), (n // 2, P_LIMBS), (n - 1, ZV), (1, [0] * 10), (n - 2, P_LIMBS)):
                xs[t], vecs[t] = 0, list(z)
            L = (n + G - 1) // G
            for i in range(L):
                mine = [t for t in (i + j * L for j in range(G)) if t < n]
                words = sum((vecs[t] for t in mine), [])

                def chk(o, mine=mine, xs=xs):
                    for j, t in enumerate(mine):
                        r = o[10 * j:10 * j + 10]
                        assert val(r) % P == (pow(xs[t], -1, P) if xs[t] else 0), f"element {t}"
                        assert reduced(r), f"bound {t}"
                    assert int(o[160]) == 0, "wrote outside the lane's elements"
                C.add(F, FE_BATCH_INV, words, (2,), p2=G, p3=n | (i << 8) | ((i & 1) << 16), check=chk,
                      desc=f"fe_batch_inv_lane<{G}> N={n} lane {i}")


def _bytes(C, rg):
    F = "bytes_sec1"
    vals = [0, 1, P - 1, P, P + 1, 2**256 - 1, N - 1, N, N + 1, 2**255, rg.getrandbits(256), rg.getrandbits(256)]
    for k, x in enumerate(vals):
        for mod in range(16):
            if (k + mod) % 3:     # two thirds of the offsets per value, every offset for some value
                continue
            off = C.put_bytes(x.to_bytes(32, "big"), mod)

            def be_chk(o, x=x):
                assert wval(o[:8]) == x

            def fe_chk(o, x=x):
                assert [int(v) for v in o[:10]] == limbs(x) and int(o[10]) == (x < P)

            def sc_chk(o, x=x):
                assert wval(o[:8]) == x and int(o[8]) == (x < N)
            C.add(F, BE32_TO_LIMBS, p2=off, check=be_chk, desc=f"be32_to_limbs @{mod}")
            C.add(F, FE_FROM_BE, p2=off, check=fe_chk, desc=f"fe_from_be @{mod}")
            C.add(F, SC_FROM_BE, p2=off, check=sc_chk, desc=f"sc_from_be @{mod}")

            def out_chk(o, x=x):
                assert struct.pack("<8I", *map(int, o[:8])) == x.to_bytes(32, "big")
            C.add(F, LIMBS_TO_BE32, w8(x), p3=(mod * 7) % 16, check=out_chk, desc=f"limbs_to_be32 @{mod}")
    # SEC1: every prefix over valid and invalid x
    pts = [O.G, O.pt_mul(O.G, 2)] + [O.pt_mul(O.G, rg.getrandbits(256)) for _ in range(3)]
    nonres_x = []
    while len(nonres_x) < 2:
        x = rg.randrange(P)
        if pow((x**3 + 7) % P, (P - 1) // 2, P) == P - 1:
            nonres_x.append(x)
    xs = [p[0] for p in pts] + [0, P - 1, P, 2**256 - 1] + nonres_x
    k = 0
    for x in xs:
        for tag in (0x02, 0x03, 0x00, 0x01, 0x04, 0xFF):
            enc = bytes([tag]) + x.to_bytes(32, "big")
            if enc == bytes(33):
                exp = bytes(64)
            else:
                try:
                    exp = O.pt_to_xy64(O.pt_from_bytes(enc))
                except ValueError:
                    exp = (1).to_bytes(32, "big") + bytes(32)
            off = C.put_bytes(enc, k % 16)

            def sec1_chk(o, exp=exp):
                assert struct.pack("<16I", *map(int, o[:16])) == exp
            C.add(F, SEC1_DECOMPRESS, p2=off, p3=(k * 5) % 16, check=sec1_chk, desc=f"sec1 {tag:02x}")
            k += 1
    off = C.put_bytes(bytes(33), 3)

    def id_chk(o):
        assert not any(int(w) for w in o[:16])
    C.add(F, SEC1_DECOMPRESS, p2=off, p3=0, check=id_chk, desc="sec1 identity")


def _proj(pnt, rg, mags, z=None):
    """Raw limbs of a projective representation of the affine point pnt (None = identity (0 : y : 0)) at magnitudes <= mags."""
    if pnt is None:
        y = z if z is not None else rg.randrange(1, P)
        X, Y, Z = 0, y, 0
    else:
        z = z if z is not None else rg.randrange(1, P)
        X, Y, Z = pnt[0] * z % P, pnt[1] * z % P, z
    return rep(X, mags[0], rg) + rep(Y, mags[1], rg) + rep(Z, mags[2], rg)


def _group(C, rg):
    F = "group"
    M5 = 5 | (2 << 8) | (2 << 16)
    endo = lambda p: None if p is None else (BETA * p[0] % P, p[1])
    G2 = O.pt_mul(O.G, 2)
    R = [O.pt_mul(O.G, rg.getrandbits(256)) for _ in range(3)]
    named = [O.G, G2, O.pt_neg(O.G), endo(O.G)] + R + [endo(R[0]), O.pt_neg(endo(R[1]))]
    assert endo(O.G) == O.pt_mul(O.G, LAM)
    # operands: (affine value, raw limbs); the identity as (0:1:0), (0:lambda:0) and with X, Z limbs equal to p
    ops = [(None, limbs(0) + limbs(1) + limbs(0)), (None, limbs(0) + limbs(LAM % P) + limbs(0)),
           (None, P_LIMBS + rep(7, 2, rg) + P_LIMBS)]
    ops += [(p, _proj(p, rg, (5, 2, 2))) for p in named]
    ops += [(named[0], noncanon(O.GX, 4) + noncanon(O.GY, 1) + noncanon(1, 1))]
    ops += [(R[0], _proj(R[0], rg, (5, 2, 2), z=LAM % P))]       # a lambda-scaled copy of R0: R0 + it is a doubling

    def result_check(exp, expect_eq, mags=(5, 2, 2), raw=None):
        def chk(o):
            X, Y, Z = (val(o[10 * c:10 * c + 10]) % P for c in range(3))
            for c in range(3):
                assert mag_ok(o[10 * c:10 * c + 10], mags[c]), f"coordinate {c} magnitude"
            if raw is not None:
                assert [int(w) for w in o[:30]] == raw, "skipped addition returns p unchanged"
            if exp is None:
                assert Z == 0 and X == 0 and Y != 0, "identity"
            else:
                zi = pow(Z, -1, P)
                assert (X * zi % P, Y * zi % P) == exp, "value"
            ax, ay = o[30:40], o[40:50]
            assert reduced(ax) and reduced(ay), "pt_to_affine bound"
            assert (val(ax) % P, val(ay) % P) == ((0, 0) if exp is None else exp), "pt_to_affine"
            assert int(o[50]) == int(expect_eq), "pt_eq"
        return chk

    def e_words(exp, k):
        """Canonical projective limbs to compare the result with: the expected point at a random scale, or (every third) another."""
        if k % 3 == 2:
            other = O.pt_add(exp, O.G)
            return _proj(other, rg, (1, 1, 1)), False
        return _proj(exp, rg, (1, 1, 1)), True

    k = 0
    for pa, wa in ops:
        for pb, wb in ops:
            exp = O.pt_add(pa, pb)
            ew, eq = e_words(exp, k)
            C.add(F, PT_ADD, wa + wb + ew, (5, 2, 2), p2=M5, check=result_check(exp, eq), desc="pt_add")
            k += 1
        exp = O.pt_add(pa, pa)
        ew, eq = e_words(exp, k)
        C.add(F, PT_DBL, wa + [0] * 30 + ew, (5, 2, 2), check=result_check(exp, eq), desc="pt_dbl")
        k += 1
    # P + (-P) and P + P at other scalings
    for p in named[:5]:
        for q in (p, O.pt_neg(p)):
            exp = O.pt_add(p, q)
            ew, eq = e_words(exp, k)
            C.add(F, PT_ADD, _proj(p, rg, (5, 2, 2)) + _proj(q, rg, (5, 2, 2)) + ew, (5, 2, 2), p2=M5,
                  check=result_check(exp, eq), desc="pt_add P+-P")
            k += 1
    # mixed additions: q affine (magnitude 1); pt_madd_nonid needs q != identity, pt_madd skips the identity sentinel
    affs = named + [O.pt_neg(named[4])]
    for pa, wa in ops:
        for q in affs[:: 2] + [pa] if pa is not None else affs[::2]:
            exp = O.pt_add(pa, q)
            qw = limbs(q[0]) + limbs(q[1])
            ew, eq = e_words(exp, k)
            C.add(F, PT_MADD_NONID, wa + qw + [0] * 10 + ew, (5, 2, 2), p2=1 | (1 << 8), check=result_check(exp, eq),
                  desc="pt_madd_nonid")
            C.add(F, PT_MADD, wa + qw + [0] * 10 + ew, (5, 2, 2), p2=1 | (1 << 8), p3=0, check=result_check(exp, eq), desc="pt_madd")
            k += 1
        ew, eq = e_words(pa, k)
        C.add(F, PT_MADD, wa + [0] * 30 + ew, (5, 2, 2), p2=1 | (1 << 8), p3=1, check=result_check(pa, eq, raw=wa), desc="pt_madd skip")
        k += 1


OFF4 = int("8" * 33, 16)


def glv_model(k):
    """The split glv_decompose computes, in big integers from the lattice basis: c_i = round(k g_i / 2^384) with
    g1 = round(2^384 b2 / n), g2 = round(2^384 (-b1) / n); k2 = -(c1 b1 + c2 b2) mod n; k1 = k - k2 lambda mod n."""
    b1, b2 = -0xE4437ED6010E88286F547FA90ABFE4C3, 0x3086D221A7D46BCDE86C90E49284EB15
    rnd = lambda x: (2 * x + N) // (2 * N)
    g1, g2 = rnd(2**384 * b2), rnd(2**384 * -b1)
    c1, c2 = (k * g1 + 2**383) >> 384, (k * g2 + 2**383) >> 384
    r2 = (-(c1 * b1) - c2 * b2) % N
    r1 = (k - r2 * LAM) % N
    return r1, r2


def _glv_scalars(rg):
    a1, b1 = 0x3086D221A7D46BCDE86C90E49284EB15, -0xE4437ED6010E88286F547FA90ABFE4C3
    a2, b2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8, 0x3086D221A7D46BCDE86C90E49284EB15
    corners = [((u * a1 + v * a2) // 2 + (u * b1 + v * b2) // 2 * LAM + d) % N for u in (-1, 1) for v in (-1, 1) for d in range(-3, 4)]
    structured = [(i * N) // 64 + j for i in range(64) for j in (-1, 0, 1)] + [(1 << i) % N for i in range(0, 256, 7)]
    ks = [0, 1, 2, N - 1, N // 2, LAM, N - LAM, 2**128, 2**255] + corners + [x % N for x in structured] + \
         [rg.randrange(N) for _ in range(200)]
    return ks


def _glv(C, rg):
    F = "glv"
    ks = _glv_scalars(rg)

    def chk(o, k):
        k1, k2 = wval(o[0:5]), wval(o[5:10])
        neg1, neg2 = int(o[10]), int(o[11])
        h1, h2 = k1 - OFF4, k2 - OFF4           # the 0x88..8 recoding offset (33 nibbles) is applied
        assert 0 <= h1 < 2**128 and 0 <= h2 < 2**128, "halves below 2^128"
        s1, s2 = (-h1 if neg1 else h1), (-h2 if neg2 else h2)
        assert (s1 + s2 * LAM) % N == k, "k1 + k2 lambda = k"
        r1, r2 = glv_model(k)
        assert (s1 % N, s2 % N) == (r1, r2), "the rounded lattice split"
    for k in ks:
        C.add(F, GLV, w8(k), check=lambda o, k=k: chk(o, k), desc="glv_decompose")


# ---------------------------------------------------------------- accumulator programs (ptj_dbl, ptj_madd, ptz_madd, ptj_to_pt, ptz_to_pt)
JAC, XYZZ = 0, 1
NOPROBE = 0xFF
OFF5 = sum(16 << (5 * i) for i in range(26))


def rep_top(x, m):
    """x mod p with every limb within one magnitude-1 step of the bound of magnitude m."""
    base = maxv(m - 1) if m > 1 else [0] * 10
    return vadd(limbs((x - val(base)) % P), base)


def negrep(y):
    """y as fe_neg_m<1> of the canonical limbs of -y leaves it: 4p - (p - y), magnitude 2 (a table entry taken with a negative digit)."""
    return [4 * pl - l for pl, l in zip(P_LIMBS, limbs((P - y) % P))]


def endo(p):
    return None if p is None else (BETA * p[0] % P, p[1])


def acc_model(steps, ops, start):
    """The accumulator as a group element: after every step (sum, empty, met an exceptional addition)."""
    S, empty, bad, trace = start, start is None, False, []
    for st in steps:
        if st[0] == "d":
            if not empty and not bad:
                S = O.pt_add(S, S)
        elif not st[2]:
            q = ops[st[1]]
            if empty:
                S, empty = q, False
            elif not bad:
                if S[0] == q[0]:
                    bad = True            # acc = q or acc = -q: H = 0 (P = 0), Z3 (ZZ3) = 0 from here on
                else:
                    S = O.pt_add(S, q)
        trace.append((S, empty, bad))
    return trace


def _accum(C, rg):
    F = "accum"
    rp = lambda: O.pt_mul(O.G, rg.randrange(1, N))

    def add(kind, steps, ops, desc, start=None, probe=NOPROBE, zmag=1):
        assert len(steps) <= 12 and len(ops) <= 4
        sb = [0] * 12
        for i, st in enumerate(steps):
            sb[i] = 0 if st[0] == "d" else (st[1] | (int(st[2]) << 2) | (1 << 4))
        words = [sum(sb[4 * w + k] << (8 * k) for k in range(4)) for w in range(3)] + [0]
        for k in range(4):
            q = ops[k] if k < len(ops) else O.G
            words += limbs(q[0]) + (negrep(q[1]) if (k + len(steps)) & 1 else limbs(q[1]))
        mags = ()
        if start is not None:
            z = rg.randrange(1, P)
            if kind == JAC:
                mags = (6, 3, 2)
                words += rep_top(start[0] * z * z, 6) + rep_top(start[1] * z**3, 3) + rep_top(z, 2)
            else:
                mags = (6, 3, zmag, zmag)
                words += rep_top(start[0] * z * z, 6) + rep_top(start[1] * z**3, 3) + rep_top(z * z, zmag) + rep_top(z**3, zmag)
        trace = acc_model(steps, ops, start)
        # Z of the Jacobian law: a product doubled (2) or a product (1); ZZ of the XYZZ law: a product (1)
        # after an addition that was carried out, afterwards 1; a skipped step keeps the raw start's (zmag)
        added = [any(st[0] == "a" and not st[2] for st in steps[:s_ + 1]) for s_ in range(len(steps))]
        zbound = [2 if kind == JAC else (1 if a else zmag) for a in added]

        def chk(o):
            for s_, (S, empty, bad) in enumerate(trace):
                z_ = o[31 + 10 * s_:41 + 10 * s_]
                assert mag_ok(z_, zbound[s_]), f"Z magnitude after step {s_}"
                if bad:
                    assert val(z_) % P == 0, f"Z = 0 after step {s_} (exceptional addition before)"
                elif not empty:
                    assert val(z_) % P != 0, f"Z != 0 after step {s_}"
            S, empty, bad = trace[-1] if trace else (start, start is None, False)
            assert int(o[30]) == int(empty), "empty"
            for c in range(3):
                assert mag_ok(o[10 * c:10 * c + 10], 1), f"converted coordinate {c} magnitude"
            X, Y, Z = (val(o[10 * c:10 * c + 10]) % P for c in range(3))
            if bad:
                return                    # the sum is re-done by the caller: only the zero Z is promised
            if empty:
                assert (X, Y, Z) == (0, 1, 0), "identity of the empty accumulator"
            else:
                zi = pow(Z, -1, P)
                assert (X * zi % P, Y * zi % P) == S, "value"
            if probe != NOPROBE:
                bounds = (6, 3, 2) if kind == JAC else (6, 3, zmag, zmag)
                for c, b in enumerate(bounds):
                    assert mag_ok(o[151 + 10 * c:161 + 10 * c], b), f"raw coordinate {c} magnitude"
        C.add(F, ACCUM, words, mags, p2=kind | (len(steps) << 8) | (int(start is not None) << 16) | (probe << 24), check=chk, desc=desc)
        return len(C.recs) - 1, trace

    D, A = ("d",), (lambda i, skip=False: ("a", i, skip))
    for rnd in range(6):
        Pn = [rp() for _ in range(4)]
        # -- Jacobian
        add(JAC, [A(0), D, D, D, D, D, A(1), A(2, True), D, D, A(3)], Pn, "ptj chain")
        add(JAC, [A(0), D, D, D, D, D, A(1), D, D, D, D, D], Pn, "ptj 5-doubling windows")
        add(JAC, [A(0, True), A(1, True), D, A(2), D, A(3)], Pn, "ptj skips on the empty accumulator, then an addition")
        add(JAC, [A(0)], Pn, "ptj first addition: the operand itself")
        add(JAC, [A(1), A(0, True)], Pn, "ptj first addition, then a skip")
        add(JAC, [], Pn, "ptj empty program")
        mid = [A(0), D, A(1), A(2, True), D, A(3)]
        i, _ = add(JAC, mid, Pn, "ptj skip in the middle (probe before)", probe=2)
        j, _ = add(JAC, mid, Pn, "ptj skip in the middle (probe at)", probe=3)
        C.same_probe.append((i, j))
        for sign in (1, -1):
            sg = (lambda q: q) if sign == 1 else O.pt_neg
            tag = "acc = q" if sign == 1 else "acc = -q"
            _, tr = add(JAC, [A(0), A(1), D, A(2), A(3, True), D, A(2)], [Pn[0], sg(Pn[0]), Pn[2], Pn[3]], f"ptj {tag} at the first step")
            assert tr[1][2] and all(t[2] for t in tr[1:])
            k = 1 + rnd % 5
            Q = O.pt_mul(Pn[0], 2**k)
            _, tr = add(JAC, [A(0)] + [D] * k + [A(1), D, A(2), A(3, True), A(2), D], [Pn[0], sg(Q), Pn[2], Pn[3]],
                        f"ptj {tag} in the middle, after {k} doublings, more points follow")
            assert not tr[k][2] and all(t[2] for t in tr[k + 1:])
            _, tr = add(JAC, [A(0), A(2)] + [D] * 5 + [A(1)], [Pn[0], sg(O.pt_mul(O.pt_add(Pn[0], Pn[2]), 32)), Pn[2]],
                        f"ptj {tag} at the last step, after 5 doublings")
            assert not tr[-2][2] and tr[-1][2]
            _, tr = add(JAC, [A(0), D, A(1)], [sg(Pn[1]), O.pt_mul(Pn[1], 2)], f"ptj {tag} from a raw start", start=Pn[1])
            assert tr[0][2]
        _, tr = add(JAC, [A(0), A(1), D, A(2)], [Pn[0], endo(Pn[0]), endo(O.pt_mul(O.pt_add(Pn[0], endo(Pn[0])), 2))],
                    "ptj operand beta x: same y, not exceptional")
        assert not any(t[2] for t in tr)
        add(JAC, [D, A(0), D, D, D, D, D, A(1), A(2, True), D, A(3)], Pn, "ptj raw start at the magnitude bounds", start=rp())
        add(JAC, [A(0, True), D, A(1)], Pn, "ptj raw start, skip first", start=rp(), probe=0)
        # -- XYZZ
        add(XYZZ, [A(0), A(1), A(2, True), A(3), A(0), A(2)], Pn, "ptz chain")
        add(XYZZ, [A(0, True), A(1, True), A(2), A(3)], Pn, "ptz skips on the empty accumulator, then an addition")
        add(XYZZ, [A(0)], Pn, "ptz first addition: the operand itself")
        add(XYZZ, [], Pn, "ptz empty program")
        mid = [A(0), A(1), A(2, True), A(3)]
        i, _ = add(XYZZ, mid, Pn, "ptz skip in the middle (probe before)", probe=1)
        j, _ = add(XYZZ, mid, Pn, "ptz skip in the middle (probe at)", probe=2)
        C.same_probe.append((i, j))
        for sign in (1, -1):
            sg = (lambda q: q) if sign == 1 else O.pt_neg
            tag = "acc = q" if sign == 1 else "acc = -q"
            _, tr = add(XYZZ, [A(0), A(1), A(2), A(3, True), A(2)], [Pn[0], sg(Pn[0]), Pn[2], Pn[3]], f"ptz {tag} at the first step")
            assert all(t[2] for t in tr[1:])
            _, tr = add(XYZZ, [A(0), A(1), A(2), A(3), A(0, True), A(3)], [Pn[0], Pn[1], sg(O.pt_add(Pn[0], Pn[1])), Pn[3]],
                        f"ptz {tag} in the middle, more points follow")
            assert not tr[1][2] and all(t[2] for t in tr[2:])
            _, tr = add(XYZZ, [A(0), A(1), A(3), A(2)], [Pn[0], Pn[1], sg(O.pt_add(O.pt_add(Pn[0], Pn[1]), Pn[3])), Pn[3]],
                        f"ptz {tag} at the last step")
            assert not tr[-2][2] and tr[-1][2]
            _, tr = add(XYZZ, [A(0), A(1)], [sg(Pn[1]), Pn[2]], f"ptz {tag} from a raw start", start=Pn[1], zmag=1 + rnd % 2)
            assert tr[0][2]
        _, tr = add(XYZZ, [A(0), A(1), A(2)], [Pn[0], endo(Pn[0]), Pn[2]], "ptz operand beta x: same y, not exceptional")
        assert not any(t[2] for t in tr)
        add(XYZZ, [A(0), A(1), A(2, True), A(3)], Pn, "ptz raw start at the magnitude bounds", start=rp(), probe=2, zmag=1 + rnd % 2)
    # a run of XYZZ programs of ONE shape (four additions, no raw start): wavefronts of the sorted device run made of these alone execute
    # ptz_madd with every lane active, and its wave_any(skip) branch is taken because SOME lanes skip
    Pn = [rp() for _ in range(4)]
    for k in range(130):
        skips = [(k * 7 + 3 * t_) % 5 == 0 for t_ in range(4)]
        add(XYZZ, [A(t_, skips[t_]) for t_ in range(4)], Pn, "ptz uniform wavefront, mixed skips")


def _recode(C, rg):
    F = "recode"

    def digits_check(o, st, signed_half):
        h = abs(signed_half)
        assert wval(o[5 * st:5 * st + 5]) == h + OFF5, f"stream {st}: glv_recode5 words"
        total = 0
        for i in range(26):
            b = (int(o[50 + 7 * st + i // 4]) >> (8 * (i % 4))) & 0xFF
            mag, neg = b & 0x7F, b >> 7
            assert mag <= 16, f"stream {st} window {i}: digit magnitude {mag} beyond the 16 table entries"
            total += (-mag if neg else mag) << (5 * i)
        assert total == signed_half, f"stream {st}: the 26 digits do not rebuild the half-scalar"

    ks = _glv_scalars(random.Random(1008))
    n0, groups = 0, []
    while n0 < len(ks):                         # groups of 1, 2, .. 5, 1, .. scalars, each scalar in exactly one group (the last wraps round)
        M = 1 + len(groups) % 5
        groups.append([(n0 + j) % len(ks) for j in range(M)])
        n0 += M
    assert {i for grp in groups for i in grp} == set(range(len(ks))), "every scalar of the _glv list is recoded"
    for idx in groups:
        M = len(idx)
        grp = [ks[i] for i in idx]

        def chk(o, grp=grp):
            for j, k in enumerate(grp):
                r1, r2 = glv_model(k)
                s1, s2 = (r1 if r1 < 2**129 else r1 - N), (r2 if r2 < 2**129 else r2 - N)
                assert (s1 + s2 * LAM) % N == k
                assert int(o[120 + 2 * j]) == int(s1 < 0) and int(o[121 + 2 * j]) == int(s2 < 0), "sign flags"
                digits_check(o, 2 * j, s1)
                digits_check(o, 2 * j + 1, s2)
        C.add(F, RECODE, sum((w8(k) for k in grp), []), p2=M, p3=1, check=chk, desc=f"recode M={M} from scalars")
    top = 2**128 - 1
    nib = [int(c * 32, 16) for c in "078F"]
    mixed = [int("".join(rg.choice("078F") for _ in range(32)), 16) for _ in range(24)]
    win = [sum(v << (5 * i) for i in range(26)) & top for v in (15, 16, 17, 31, 1)]                 # every 5-bit window at one value
    carry = [top - (1 << b) for b in (0, 4, 5, 64, 120, 124, 125, 127)] + [(1 << b) - 1 for b in (120, 124, 125, 126, 127)] + \
            [(top - OFF5) % 2**128, (top - OFF5 + 1) % 2**128, (2**130 - 1 - OFF5) % 2**128, 2**127, 2**125, 2**125 - 16]
    halves = [0, top] + nib + mixed + win + carry + [rg.getrandbits(128) for _ in range(20)]
    pairs = [(0, h) for h in halves[:12]] + [(h, 0) for h in halves[:12]] + [(top, h) for h in halves[:8]] + [(h, top) for h in halves[:8]] + \
            [(0, 0), (top, top), (0, top), (top, 0)] + [(halves[i], halves[-1 - i]) for i in range(len(halves))]
    n0, groups = 0, []
    while n0 < len(pairs):
        M = 1 + len(groups) % 5
        groups.append([(n0 + j) % len(pairs) for j in range(M)])
        n0 += M
    assert {i for grp in groups for i in grp} == set(range(len(pairs))), "every pair of half-scalars is recoded"
    for idx in groups:
        M = len(idx)
        grp = [pairs[i] for i in idx]
        signs = [(i & 1, (i >> 1) & 1) for i in idx]
        words = []
        for (h1, h2), (n1, n2) in zip(grp, signs):
            for h in (h1, h2):
                words += [((h + OFF4) >> (32 * i)) & 0xFFFFFFFF for i in range(5)]
            words += [n1, n2]

        def chk(o, grp=grp, signs=signs):
            for j, ((h1, h2), (n1, n2)) in enumerate(zip(grp, signs)):
                assert int(o[120 + 2 * j]) == n1 and int(o[121 + 2 * j]) == n2, "sign flags"
                digits_check(o, 2 * j, -h1 if n1 else h1)
                digits_check(o, 2 * j + 1, -h2 if n2 else h2)
        C.add(F, RECODE, words, p2=M, p3=0, check=chk, desc=f"recode M={M} from half-scalars")


def split_begin(parts, part):
    """The test's own copy of straus_core.h's split_begin (the records name a cut and the dispatcher calls the C one; out[192] must
    agree with this one): the first window of part `part` of a 26-window stream cut in `parts`.  Production cuts a stream in 2 or 4
    (BPPP_SPLIT_PARTS_MAX); any other count falls into the 4-part branch, with 26 for every part past the fourth."""
    if parts == 1:
        return 0 if part == 0 else 26
    if parts == 2:
        return (0, 13, 26)[min(part, 2)]
    return (0, 7, 14, 20, 26)[min(part, 4)]


def _table(C, rg):
    F = "table"
    # 8 parts is no production cut: it reuses the 4-part branch and adds 130 doublings (part >= 4), a table no caller builds but a
    # well-formed input to affine_table_one
    cuts = [(1, 0), (2, 0), (2, 1), (4, 0), (4, 1), (4, 2), (4, 3), (8, 0), (8, 1), (8, 2), (8, 3), (8, 4), (8, 7)]
    assert {5 * split_begin(*c) for c in cuts} == {0, 35, 65, 70, 100, 130}
    for name, pnt in (("G", O.G), ("random point", O.pt_mul(O.G, rg.randrange(1, N))), ("identity sentinel", None)):
        for parts, part in cuts:
            pre = 5 * split_begin(parts, part)
            base = None if pnt is None else O.pt_mul(pnt, 2**pre)
            for first in (1, 9):
                def chk(o, base=base, first=first, pre=pre):
                    assert int(o[192]) == pre, "doublings done first"
                    assert int(o[193]) == 0, "aff_ld returns the stored words"
                    for k in range(8):
                        x, y, bx = (wval(o[24 * k + 8 * c:24 * k + 8 * c + 8]) for c in range(3))
                        if base is None:
                            assert (x, y, bx) == (0, 0, 0), f"entry {first + k} of the sentinel's table is the sentinel"
                            continue
                        e = O.pt_mul(base, first + k)
                        assert (x, y) == e, f"entry {first + k}"
                        assert bx == BETA * x % P, f"entry {first + k}: beta x"
                        if k == (first + pre) % 8:
                            assert (bx, y) == O.pt_mul(e, LAM), f"entry {first + k}: the beta-frame twin is lambda times the entry"
                xy = limbs(pnt[0]) + limbs(pnt[1]) if pnt else [0] * 20
                C.add(F, TABLE, xy, (1, 1), p2=parts | (part << 8), p3=first, check=chk,
                      desc=f"affine_table_one {name}, part {part} of {parts} ({pre} doublings), entries {first}..{first + 7}")


def _draw(C, rg):
    F = "draw"
    for i in range(16):
        key = bytes(rg.getrandbits(8) for _ in range(32)) if i else bytes(32)
        stream = (0, 1, 2**32, 2**64 - 1)[i % 4] if i < 8 else rg.getrandbits(64)
        counter = (0, 1, 2**32 - 1, 2**32, 2**64 - 1)[i % 5] if i < 10 else rg.getrandbits(64)
        exp = chacha_ref.draw(key, stream, counter).to_bytes(32, "big")
        words = list(struct.unpack("<8I", key)) + [stream & 0xFFFFFFFF, stream >> 32, counter & 0xFFFFFFFF, counter >> 32]

        def chk(o, exp=exp):
            assert struct.pack("<8I", *map(int, o[:8])) == exp
        C.add(F, DRAW_SCALAR, words, check=chk, desc="draw_scalar_words")


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        C = Cases()
        for i, gen in enumerate((_fe_products, _fe_linear, _fe_normalize, _fn, _fn_wrap, _inversion, _bytes, _group, _glv, _draw,
                                 _accum, _recode, _table)):
            gen(C, random.Random(1000 + i))
        _CASES = C
    return _CASES


# ---------------------------------------------------------------- backends
def _aligned_bytes(data):
    buf = np.zeros(len(data) + 64, np.uint8)
    start = (-buf.ctypes.data) % 64
    view = buf[start:start + len(data)]
    view[:] = np.frombuffer(bytes(data), np.uint8)
    return buf, view


def _run(L, recs, data):
    recs = np.ascontiguousarray(recs, dtype=np.uint32)
    out = np.zeros((len(recs), OUT_W), np.uint32)
    keep, view = _aligned_bytes(data)
    rc = L.run(recs.ctypes.data, out.ctypes.data, len(recs), view.ctypes.data, len(view))
    assert rc == 0, f"run returned {rc}"
    return out


_OUT, _SORTED = {}, {}


def outputs(backend):
    if backend not in _OUT:
        why = PB.unavailable(backend)
        if why:
            pytest.skip(f"{backend} backend skipped: {why}")
        L = PB.load(backend)
        assert (L.prims_record_words(0), L.prims_record_words(1)) == (IN_W, OUT_W)
        if backend != "gfx950":
            assert L.prims_is_clang() == (backend == "clang")
        C = cases()
        recs = np.array(C.recs, dtype=np.uint32)
        if backend == "gfx950":
            # shuffled: every wavefront mixes op codes and byte offsets; sorted by op code: uniform wavefronts
            perm = np.random.default_rng(7).permutation(len(recs))
            out = np.empty((len(recs), OUT_W), np.uint32)
            out[perm] = _run(L, recs[perm], C.bytes)
            order = np.argsort(recs[:, 0], kind="stable")
            srt = np.empty_like(out)
            srt[order] = _run(L, recs[order], C.bytes)
            _SORTED[backend] = srt
        else:
            out = _run(L, recs, C.bytes)
        _OUT[backend] = out
    return _OUT[backend]


BACKEND_PARAMS = ["gcc", "clang", pytest.param("gfx950", marks=pytest.mark.gpu)]


@pytest.fixture(scope="module", params=BACKEND_PARAMS)
def backend(request):
    return request.param


@pytest.mark.parametrize("family", FAMILIES)
def test_primitives(backend, family):
    """Value and promise of every record of one op family on one build."""
    out = outputs(backend)
    C = cases()
    bad, n = [], 0
    for i, (fam, check, desc) in enumerate(C.meta):
        if fam != family:
            continue
        n += 1
        try:
            assert int(out[i, OUT_W - 1]) == 0, f"status {int(out[i, OUT_W - 1])}"
            check(out[i])
        except AssertionError as e:
            bad.append(f"#{i} {desc}: {e}")
    assert n > 0
    assert not bad, f"{len(bad)} of {n} {family} records wrong on {backend}:\n" + "\n".join(bad[:20])


def test_same_bits_everywhere(backend):
    """The raw output words of every record are identical across the builds (not merely congruent)."""
    out = outputs(backend)
    C = cases()
    others = [b for b in ("gcc", "clang") if b != backend and PB.unavailable(b) is None]
    if not others:
        pytest.skip("no second build to compare with")
    for other in others:
        diff = np.nonzero((out != outputs(other)).any(axis=1))[0]
        assert len(diff) == 0, f"{backend} vs {other}: {len(diff)} records differ, first: " + \
            "; ".join(f"#{i} {C.meta[i][2]}" for i in diff[:10])
    if backend == "gfx950":
        diff = np.nonzero((out != _SORTED[backend]).any(axis=1))[0]
        assert len(diff) == 0, f"shuffled vs sorted device runs: {len(diff)} records differ, first: " + \
            "; ".join(f"#{i} {C.meta[i][2]}" for i in diff[:10])


def test_skipped_step_keeps_the_raw_limbs(backend):
    """A skipped addition in the middle of an accumulator program leaves every raw limb as it was: the same program probed before and
    at the skipped step."""
    out = outputs(backend)
    C = cases()
    assert len(C.same_probe) >= 12
    for i, j in C.same_probe:
        assert int(out[i, OUT_W - 1]) == 0 and int(out[j, OUT_W - 1]) == 0
        assert out[i, 151:191].any(), C.meta[i][2]
        assert (out[i, 151:191] == out[j, 151:191]).all(), f"#{i} / #{j} {C.meta[j][2]}"


def test_dispatcher_rejects_out_of_range_records(backend):
    """The new ops keep the dispatcher's guards: a step count, step code, probe index, recoding size or table part out of range is
    answered with ST_BAD_PARAM (2) and no evaluation."""
    why = PB.unavailable(backend)
    if why:
        pytest.skip(f"{backend} backend skipped: {why}")
    xy = limbs(O.GX) + limbs(O.GY)
    bad = [(ACCUM, JAC | (13 << 8) | (NOPROBE << 24), 0, []),              # 13 steps
           (ACCUM, 2 | (1 << 8) | (NOPROBE << 24), 0, [1 << 4]),            # no such accumulator
           (ACCUM, JAC | (1 << 8) | (1 << 24), 0, [1 << 4]),                # probe past the program
           (ACCUM, JAC | (1 << 8) | (NOPROBE << 24), 0, [2 << 4]),          # no such step
           (ACCUM, XYZZ | (1 << 8) | (NOPROBE << 24), 0, [0]),              # the XYZZ accumulator has no doubling
           (RECODE, 0, 1, []), (RECODE, 6, 1, []), (RECODE, 2, 2, []),
           (TABLE, 3, 1, xy), (TABLE, 2 | (2 << 8), 1, xy), (TABLE, 1, 5, xy)]
    recs = np.zeros((len(bad), IN_W), np.uint32)
    for r, (op, p2, p3, words) in zip(recs, bad):
        r[0], r[2], r[3] = op, p2, p3
        r[4:4 + len(words)] = words
    out = _run(PB.load(backend), recs, bytes(64))
    assert out[:, OUT_W - 1].tolist() == [2] * len(bad)
    assert not out[:, :OUT_W - 1].any()


def test_sorted_run_mixes_skips_in_a_wavefront():
    """The record set itself: in the device run sorted by op code, some wavefront is made of XYZZ programs of one shape alone with
    skipping and adding lanes side by side (ptz_madd's wave_any(skip) branch under a full exec mask), and some wavefront holds such
    lanes next to programs of another shape (the same branch under a partial one)."""
    C = cases()
    recs = np.array(C.recs, dtype=np.uint32)
    order = np.argsort(recs[:, 0], kind="stable")
    full = partial = False
    for w0 in range(0, len(order), 64):
        wave = [recs[i] for i in order[w0:w0 + 64]]
        zz = [r for r in wave if r[0] == ACCUM and (r[2] & 0xFF) == XYZZ]
        if not zz:
            continue
        skip_at = [{s_ for s_ in range((int(r[2]) >> 8) & 0xFF) if (int(r[4 + s_ // 4]) >> (8 * (s_ % 4))) & 4} for r in zz]
        mixed = any(any(s_ in a for a in skip_at) and not all(s_ in a for a in skip_at) for s_ in range(12))
        one_shape = len(wave) == 64 and len(zz) == 64 and len({int(r[2]) for r in zz}) == 1
        full |= mixed and one_shape
        partial |= mixed and len({(int(r[0]), int(r[2])) for r in wave}) > 1
    assert full and partial


# ---------------------------------------------------------------- the variable-base sums on production-built tables, fallback included
SUM_AFFINE, SUM_FAST_COMPLETE, SUM_SPLIT_LANES, SUM_COMPLETE, SUM_GROUP, SUM_SPLIT_GROUP = range(6)
# (form, M, G, parts): the one-lane forms (host twins) and every lane-group form the verifiers instantiate (verify_core.h,
# recip_core.h, wnla_core.h, prove_core.h: straus_affine_g4<2 | 5, 2 | 4>, straus_affine_split<2, 8, 2>, <2, 16, 4>, <5, 32, 2>, <5, 64, 4>)
SUM_ONE_LANE = [(SUM_AFFINE, m, 1, 0) for m in (1, 2, 3, 4, 5)] + \
               [(f, m, 1, 0) for f in (SUM_FAST_COMPLETE, SUM_COMPLETE) for m in (2, 5)] + \
               [(SUM_SPLIT_LANES, m, 1, parts) for m in (2, 5) for parts in (2, 4)]
SUM_GROUPS = [(SUM_GROUP, m, g, 0) for m in (2, 5) for g in (2, 4)] + \
             [(SUM_SPLIT_GROUP, 2, 8, 2), (SUM_SPLIT_GROUP, 2, 16, 4), (SUM_SPLIT_GROUP, 5, 32, 2), (SUM_SPLIT_GROUP, 5, 64, 4)]


def sum_cfg(cfg):
    form, m, g, parts = cfg
    return form | (m << 8) | (g << 16) | (parts << 24)


def signed_halves(k):
    r1, r2 = glv_model(k)
    return (r1 if r1 < 2**129 else r1 - N), (r2 if r2 < 2**129 else r2 - N)


def stream_digits(h):
    """The 26 signed 5-bit digits of the signed half-scalar h, lowest window first."""
    w = abs(h) + OFF5
    return [(((w >> (5 * i)) & 31) - 16) * (-1 if h < 0 else 1) for i in range(26)]


def lane_meets_exception(streams, windows):
    """One lane of a sum as group elements: `streams` = [(point, digits)], walked from the last of `windows` down with 5 doublings
    between windows, skipping zero digits and identity points.  True when some addition finds acc = +-q (the incomplete law's exception)."""
    acc = None
    empty = True
    for n_, i in enumerate(reversed(windows)):
        if n_ and not empty:
            acc = O.pt_mul(acc, 32)
        for pnt, dg in streams:
            if pnt is None or dg[i] == 0:
                continue
            q = O.pt_mul(pnt, abs(dg[i]))
            q = O.pt_neg(q) if dg[i] < 0 else q
            if empty:
                acc, empty = q, False
            elif acc is None or acc[0] == q[0]:
                return True
            else:
                acc = O.pt_add(acc, q)
    return False


def sum_meets_exception(cfg, pts, ks):
    """Whether the fast form of configuration cfg meets an exceptional addition on some lane, for M points / scalars."""
    form, m, g, parts = cfg
    streams = []
    for pnt, k in zip(pts, ks):
        h1, h2 = signed_halves(k)
        streams += [(pnt, stream_digits(h1)), (endo(pnt), stream_digits(h2))]
    if form in (SUM_AFFINE, SUM_FAST_COMPLETE):
        return lane_meets_exception(streams, range(26))
    if form == SUM_GROUP:
        return any(lane_meets_exception(streams[q::g], range(26)) for q in range(g))
    if form in (SUM_SPLIT_LANES, SUM_SPLIT_GROUP):
        cut = lambda pnt, h: None if pnt is None else O.pt_mul(pnt, 2**(5 * split_begin(parts, h)))
        return any(lane_meets_exception([(cut(pnt, h), dg[split_begin(parts, h):])], range(split_begin(parts, h + 1) - split_begin(parts, h)))
                   for h in range(parts) for pnt, dg in streams)
    return False


_SUM_MEETS = {}


def sum_meets(cfg, i):
    """sum_meets_exception for record i of configuration cfg (computed once for all builds)."""
    if (cfg, i) not in _SUM_MEETS:
        _, pts, ks, _ = sum_records(cfg)[0][i]
        _SUM_MEETS[(cfg, i)] = sum_meets_exception(cfg, pts, ks)
    return _SUM_MEETS[(cfg, i)]


def sum_inputs(m):
    """(description, points, scalars, certain) for sums of m points (m <= 4 real ones; a fifth slot of the five-point forms holds the
    identity with scalar 0).  certain: the one-lane fast form must report an exception -- equal or opposite points with equal scalars
    in [2^120, 2^127) (or 1), whose lambda halves are zero, beside scalars below 2^60 (or 0), whose digits at k's first non-zero window
    are zero: the accumulator holds d P alone when the second copy's d P (or -d P) arrives."""
    rg = random.Random(4242 + m)
    real = min(m, 4)
    rp = lambda: O.pt_mul(O.G, rg.randrange(1, N))
    rs = lambda: rg.randrange(1, N)
    small = lambda: rg.randrange(2**120, 2**127)
    pad = lambda pts, ks: (pts + [None] * (m - len(pts)), ks + [0] * (m - len(ks)))
    out = []

    def add(desc, pts, ks, certain=False):
        pts, ks = pad(list(pts), list(ks))
        out.append((desc, pts, ks, certain))

    for _ in range(6):
        add("distinct points and scalars", [rp() for _ in range(real)], [rs() for _ in range(real)])
    for a in (0, 1, N - 1, LAM):
        add(f"scalar {a if a < 2 else 'n - 1' if a == N - 1 else 'lambda'} everywhere", [rp() for _ in range(real)], [a] * real)
        add("scalars 0, 1, n - 1, lambda", [rp() for _ in range(real)], [(0, 1, N - 1, LAM)[(j + a) % 4] for j in range(real)])
    add("all points the identity", [None] * real, [rs() for _ in range(real)])
    add("all scalars 0 and all points the identity", [None] * real, [0] * real)
    for j in range(real):
        pts = [rp() for _ in range(real)]
        pts[j] = None
        add(f"identity in slot {j} among real points", pts, [rs() for _ in range(real)])
    if real >= 2:
        for i in range(real):
            for j in range(i + 1, real):
                for sign in (1, -1):
                    for k, certain in ((small(), True), (rs(), False), (1, True), (N - 1, False), (LAM, False)):
                        # certain: the other points' scalars end below the window where k begins (0 beside k = 1)
                        pts, ks = [rp() for _ in range(real)], [(rg.randrange(2**60) if k > 1 else 0) if certain else rs() for _ in range(real)]
                        pts[j] = pts[i] if sign == 1 else O.pt_neg(pts[i])
                        ks[i] = ks[j] = k
                        add(f"slots {i} and {j}: {'the same point' if sign == 1 else 'P and -P'}, the same scalar", pts, ks, certain)
    if real >= 3:
        for n_same in range(3, real + 1):
            for k, certain in ((small(), True), (rs(), False)):
                pts, ks = [rp() for _ in range(real)], [rg.randrange(2**60) if certain else rs() for _ in range(real)]
                for j in range(n_same):
                    pts[j], ks[j] = pts[0], k
                add(f"the same point and scalar in {n_same} slots", pts, ks, certain)
    return out


_SUM_IN, _SUM_OUT = {}, {}


def sum_records(cfg):
    m = cfg[1]
    if m not in _SUM_IN:
        _SUM_IN[m] = sum_inputs(m)
    recs = np.zeros((len(_SUM_IN[m]), SUM_IN_W), np.uint32)
    for r, (_, pts, ks, _) in zip(recs, _SUM_IN[m]):
        r[0] = sum_cfg(cfg)
        for j, (pnt, k) in enumerate(zip(pts, ks)):
            if pnt is not None:
                r[4 + 16 * j:4 + 16 * j + 16] = w8(pnt[0]) + w8(pnt[1])
            r[84 + 8 * j:84 + 8 * j + 8] = w8(k)
    return _SUM_IN[m], recs


def sum_outputs(backend, cfg):
    if (backend, cfg) not in _SUM_OUT:
        why = PB.unavailable(backend)
        if why:
            pytest.skip(f"{backend} backend skipped: {why}")
        L = PB.load(backend)
        assert (L.prims_sum_words(0), L.prims_sum_words(1)) == (SUM_IN_W, SUM_OUT_W)
        _, recs = sum_records(cfg)
        out = np.zeros((len(recs), SUM_OUT_W), np.uint32)
        rc = L.run_sums(sum_cfg(cfg), recs.ctypes.data, out.ctypes.data, len(recs))
        assert rc == 0, f"run_sums returned {rc}"
        _SUM_OUT[(backend, cfg)] = out
    return _SUM_OUT[(backend, cfg)]


_SUM_EXPECT = {}


def sum_expected(m):
    if m not in _SUM_EXPECT:
        exp = []
        for _, pts, ks, _ in sum_records((SUM_AFFINE, m, 1, 0))[0]:
            total = None
            for pnt, k in zip(pts, ks):
                total = O.pt_add(total, O.pt_mul(pnt, k))
            exp.append(total)
        _SUM_EXPECT[m] = exp
    return _SUM_EXPECT[m]


def check_sums(backend, cfg):
    form, m, g, parts = cfg
    inputs, _ = sum_records(cfg)
    out = sum_outputs(backend, cfg)
    bad, fell_back = [], 0
    for i, ((desc, pts, ks, certain), exp) in enumerate(zip(inputs, sum_expected(m))):
        o = out[i]
        try:
            assert int(o[SUM_OUT_W - 1]) == 0, f"status {int(o[SUM_OUT_W - 1])}"
            for c, b in enumerate((5, 2, 2)):
                assert mag_ok(o[10 * c:10 * c + 10], b), f"coordinate {c} magnitude"
            ax, ay = o[30:40], o[40:50]
            assert reduced(ax) and reduced(ay), "pt_to_affine bound"
            assert (val(ax) % P, val(ay) % P) == ((0, 0) if exp is None else exp), "sum != sum_i k_i P_i of the oracle"
            assert int(o[72]) == 0, "lanes of the group disagree on the total"
            if form in (SUM_GROUP, SUM_SPLIT_GROUP):
                assert int(o[73]) == int(sum_meets(cfg, i)), \
                    f"the device finds {'an' if int(o[73]) else 'no'} exceptional addition in the group, the group-element model the opposite"
            if form not in (SUM_FAST_COMPLETE, SUM_SPLIT_LANES):
                assert int(o[50]) == 2, "flag of a form that returns none"
        except AssertionError as e:
            bad.append(f"#{i} {desc}: {e}")
        if form in (SUM_FAST_COMPLETE, SUM_SPLIT_LANES):
            meets = sum_meets(cfg, i)
            fell_back += meets
            if form == SUM_FAST_COMPLETE and certain and not meets:
                bad.append(f"#{i} {desc}: constructed to meet an exceptional addition, the model finds none")
            if int(o[50]) != int(not meets):
                bad.append(f"#{i} {desc}: fast form returned {int(o[50])}, the group-element model expects {int(not meets)}")
    assert not bad, f"{len(bad)} of {len(inputs)} sums wrong for form {form} M={m} G={g} parts={parts} on {backend}:\n" + "\n".join(bad[:20])
    return fell_back


@pytest.mark.parametrize("cfg", SUM_ONE_LANE, ids=lambda c: "form%d-M%d-parts%d" % (c[0], c[1], c[3]))
def test_sums_one_lane(backend, cfg):
    """straus_affine, straus_affine_fast + straus_affine_complete, straus_affine_complete and the lanes of straus_split_lane on tables
    built by affine_tables_build / affine_table_one: every sum equals sum_i k_i P_i of the oracle, coincident and identity points
    included, and the fast forms' flag is the one a group-element model of the same lane predicts (false, with certainty, for equal
    or opposite points with equal scalars below 2^127)."""
    fell_back = check_sums(backend, cfg)
    if cfg[0] == SUM_FAST_COMPLETE:
        certain = sum(1 for rec in sum_records(cfg)[0] if rec[3])
        assert certain >= 4 and fell_back >= certain, "the records built to take the fallback take it"


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SUM_GROUPS, ids=lambda c: "form%d-M%d-G%d-parts%d" % c)
def test_sums_lane_groups(cfg):
    """straus_affine_g4<M, G> and straus_affine_split<M, G, PARTS> on their real lane groups, 64 / G independent sums per wavefront,
    exceptional groups next to ordinary ones: every sum equals the oracle's, on every lane of the group.  The record set holds sums
    whose streams meet in ONE lane (an exception, and the group-wide re-do) and sums whose streams meet across lanes or parts (the
    complete additions of the shuffle tree).  Which is which follows from the group-element model, and the kernel reports for every
    sum whether a lane of its group met an exceptional addition (recomputed beside the function under test: straus_affine_fast over
    the lane's own streams, or straus_split_lane); the two must agree record by record, so the model cannot drift from the device.

    The `if (bad)` block of straus_affine_split is NOT covered by result: a lane of a split sum walks one stream over one table, its
    accumulator is 32 A Q against an entry d Q with |d| <= 16, and in a group of prime order these never meet.  No well-formed input
    reaches that block; the test asserts that no record does."""
    check_sums("gfx950", cfg)
    if cfg[0] == SUM_GROUP:
        # lane q of a group of G holds the streams q, q + G, ...: two points' streams share a lane when 2 M > G, and with G = 4 (two
        # streams of a point, then the next point's) some pairs of points never do
        inputs, _ = sum_records(cfg)
        meets = [sum_meets(cfg, i) for i, rec in enumerate(inputs) if rec[3]]
        assert meets.count(True) >= (4 if 2 * cfg[1] > cfg[2] else 0), "sums whose coincident streams share a lane"
        assert meets.count(False) >= (4 if cfg[2] == 4 else 0), "sums whose coincident streams lie in different lanes"
    else:
        assert not any(sum_meets(cfg, i) for i in range(len(sum_records(cfg)[0]))), "a split lane never meets an exception"


def test_sums_same_bits_everywhere(backend):
    """The one-lane sums give identical raw words on every build."""
    others = [b for b in ("gcc", "clang") if b != backend and PB.unavailable(b) is None]
    if not others:
        pytest.skip("no second build to compare with")
    for cfg in SUM_ONE_LANE:
        for other in others:
            diff = np.nonzero((sum_outputs(backend, cfg) != sum_outputs(other, cfg)).any(axis=1))[0]
            assert len(diff) == 0, f"{cfg} {backend} vs {other}: records {list(diff[:10])} differ"


def test_limb_helpers():
    """The test's own constructions: ZV is 0 mod p at magnitude exactly 1, all-max vectors sit on the magnitude bound, the
    non-canonical representations keep their value."""
    assert val(P_LIMBS) == P and val(ZV) == 2 * P and mag_ok(ZV, 1) and not mag_ok([v + 1 for v in ZV], 1)
    rg = random.Random(3)
    for m in range(1, 17):
        assert mag_ok(maxv(m), m) and not mag_ok(vadd(maxv(m), [1] + [0] * 9), m)
        x = rg.randrange(P)
        assert val(noncanon(x, m - 1)) % P == x and mag_ok(noncanon(x, m - 1), m)
        assert val(rep(x, m, rg)) % P == x and mag_ok(rep(x, m, rg), m)
