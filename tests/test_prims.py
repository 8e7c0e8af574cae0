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
codes and byte offsets) and sorted by op code (uniform wavefronts); both runs must agree word for word."""
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
IN_W, OUT_W = 176, 168

# op codes: prims_core.h enum Op
FE_MUL, FE_SQR, FE_MUL2_ADD, FE_MUL_SMALL, FE_ADD, FE_SUB_M, FE_NEG_M, FE_NORMALIZE = range(1, 9)
FE_IS_ZERO, FE_IS_ODD, FE_EQ, FE_TO_W8, FE_FROM_W8, FE_INV, FE_INV_FERMAT, FE_SQRT, FE_BATCH_INV = range(9, 18)
SC_ADD, SC_SUB, SC_NEG, SC_MUL, SC_SQR, SC_REDUCE512, DRAW_REDUCE512, SC_INV, SC_INV_FERMAT = range(32, 41)
BE32_TO_LIMBS, FE_FROM_BE, SC_FROM_BE, SEC1_DECOMPRESS, LIMBS_TO_BE32 = range(48, 53)
PT_ADD, PT_DBL, PT_MADD_NONID, PT_MADD = range(64, 68)
GLV, DRAW_SCALAR = 80, 81

FAMILIES = ("fp_products", "fp_linear", "fp_normalize", "fn", "fn_wrap", "inversion", "bytes_sec1", "group", "glv", "draw")

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


def _glv(C, rg):
    F = "glv"
    a1, b1 = 0x3086D221A7D46BCDE86C90E49284EB15, -0xE4437ED6010E88286F547FA90ABFE4C3
    a2, b2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8, 0x3086D221A7D46BCDE86C90E49284EB15
    corners = [((u * a1 + v * a2) // 2 + (u * b1 + v * b2) // 2 * LAM + d) % N for u in (-1, 1) for v in (-1, 1) for d in range(-3, 4)]
    structured = [(i * N) // 64 + j for i in range(64) for j in (-1, 0, 1)] + [(1 << i) % N for i in range(0, 256, 7)]
    ks = [0, 1, 2, N - 1, N // 2, LAM, N - LAM, 2**128, 2**255] + corners + [x % N for x in structured] + \
         [rg.randrange(N) for _ in range(200)]

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
        for i, gen in enumerate((_fe_products, _fe_linear, _fe_normalize, _fn, _fn_wrap, _inversion, _bytes, _group, _glv, _draw)):
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
