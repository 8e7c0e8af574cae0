// The reciprocal range proof's witness from the integer alone: the generalisation of u64_proof.rs:84-102 (u64_to_hex,
// u64_to_hex_mapped) to runtime dim_nd / dim_np.  Per instance, from x (32 big-endian bytes):
//   digits[dim_nd]  the base-dim_np digits of x, least significant first (the order of u64_to_hex),
//   m[dim_np]       m[v] = how many digits equal v,
// as the 32-byte scalars recip_prove_stage_r1 (recip_prove_core.h) reads, and a status:
//   x >= n            RW_BAD_ENCODING  (a non-canonical scalar, as for every other input scalar), and nothing else;
//   x >= np^nd        RW_OUT_OF_RANGE  (the value has more than dim_nd digits: no witness exists).
// A flagged instance still gets the low dim_nd digits of its 256-bit value and their multiplicities -- valid scalars, so the stages
// behind this one run on it like on any other lane and flag nothing of their own accord; the host zeroes its proof and commitment.
//
// x determines its digits only while np^nd <= n (recip_values_shape_ok): above that two integers that agree mod n would have different
// digit vectors, and the entry points refuse the shape.
//
// Host and device code with no HIP in it (like draw_core.h): the kernel (k_gprove.hip: k_rprove_witness), the host side's shape check and
// the CPU tier's g++ build (tests/test_recip_values_emul.py) compile this same file.
//
// Constant time in x: one digit per pass of a fixed-length loop, by shifts (np a power of two) or by a multiplication with the
// reciprocal of np and one masked correction (any other np); the multiplicities by compare-and-accumulate over all (digit, value)
// pairs.  No branch and no address depends on x or on a digit; np, nd and the batch index are public.
#pragma once
#include "field.h"

namespace bppp {

constexpr int32_t RW_BAD_ENCODING = 1;      // = ST_BAD_ENCODING / BPPP_ST_BAD_ENCODING
constexpr int32_t RW_OUT_OF_RANGE = 4;      // = ST_OUT_OF_RANGE / BPPP_ST_OUT_OF_RANGE

struct RecipWitnessWs {
    size_t N;
    int nd, np;
    int bits;              // np = 2^bits (bits = 0: np = 1), or -1: any other np, digits by division
    u64 recip;             // floor(2^64 / np) for the division path
    const uint8_t* x;      // N x 32, big-endian
    uint8_t* digits;       // N x nd x 32
    uint8_t* m;            // N x np x 32
    int32_t* status;       // N
};

// the shape fields of a RecipWitnessWs (1 <= np <= 2^16: the entry points bound np by dim_nd + 1 <= 4097)
inline void recip_witness_shape(RecipWitnessWs& w, size_t nd, size_t np) {
    w.nd = (int)nd; w.np = (int)np;
    w.bits = -1;
    w.recip = 0;
    if ((np & (np - 1)) == 0) {
        w.bits = 0;
        while (((size_t)1 << w.bits) < np) w.bits++;
    } else {
        w.recip = ~(u64)0 / (u64)np;      // np is no power of two: floor((2^64 - 1) / np) = floor(2^64 / np)
    }
}

// np^nd <= n, the group order: the shapes whose digits x determines.  16^63, 2^255, 10^77 pass; 16^64, 2^256, 10^78 do not.
inline bool recip_values_shape_ok(size_t nd, size_t np) {
    if (nd == 0 || np == 0 || np > 0xFFFFFFFFu) return false;
    if (np == 1) return true;
    if (nd > 256) return false;           // np >= 2: 2^257 > n
    const u32 order[8] = {0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    u32 p[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < nd; i++) {
        u64 carry = 0;
        for (int l = 0; l < 8; l++) {
            const u64 v = (u64)p[l] * (u64)np + carry;
            p[l] = (u32)v;
            carry = v >> 32;
        }
        if (carry) return false;          // >= 2^256 > n
    }
    for (int l = 7; l >= 0; l--)
        if (p[l] != order[l]) return p[l] < order[l];
    return true;                          // np^nd = n (cannot happen: n is prime)
}

// the high 64 bits of a x b
HD u64 rw_mulhi64(u64 a, u64 b) {
    const u64 a0 = (u32)a, a1 = a >> 32, b0 = (u32)b, b1 = b >> 32;
    const u64 p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const u64 mid = (p00 >> 32) + (u32)p01 + (u32)p10;
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// v (8 little-endian limbs) := floor(v / np), returns v mod np
HD u32 rw_next_digit(u32 v[8], const RecipWitnessWs& w) {
    if (w.bits >= 0) {                    // (public, uniform) np = 2^bits, bits <= 16
        const u32 d = v[0] & ((u32)w.np - 1u);
        const u32 up = (u32)(32 - w.bits) & 31u, keep = w.bits ? ~0u : 0u;      // bits = 0: nothing moves
#pragma unroll
        for (int l = 0; l < 8; l++) v[l] = (v[l] >> w.bits) | (((l < 7 ? v[l + 1] : 0u) << up) & keep);
        return d;
    }
    // long division, most significant limb first: cur = rem 2^32 + limb < np 2^32, q = floor(cur / np) < 2^32.
    // qe = floor(cur recip / 2^64) is q or q - 1 (cur / np - cur recip / 2^64 = cur (2^64 - recip np) / (np 2^64) < cur / 2^64 < 1),
    // so cur - qe np is below 2 np and one subtraction of np, selected by mask, finishes the step.
    const u64 np = (u64)(u32)w.np;
    u64 rem = 0;
#pragma unroll
    for (int l = 7; l >= 0; l--) {
        const u64 cur = (rem << 32) | v[l];
        u64 qe = rw_mulhi64(cur, w.recip);
        u64 r = cur - qe * np;
        const u64 over = (u64)0 - (u64)(r >= np);
        r -= np & over;
        qe += 1u & over;
        v[l] = (u32)qe;
        rem = r;
    }
    return (u32)rem;
}

// the witness of instance t; returns its status (also written to w.status[t])
HD int32_t recip_witness(const RecipWitnessWs& w, size_t t) {
    sc xs;
    const bool canonical = sc_from_be(xs, w.x + 32 * t);
    u32 v[8];
#pragma unroll
    for (int l = 0; l < 8; l++) v[l] = xs.v[l];
    uint8_t* dig = w.digits + t * (size_t)w.nd * 32;
#pragma nounroll
    for (int i = 0; i < w.nd; i++) {
        sc d;
        sc_set_u32(d, rw_next_digit(v, w));
        sc_to_be(dig + (size_t)i * 32, d);
    }
    // what is left of x above its dim_nd digits: zero iff x < np^nd
    u32 rest = 0;
#pragma unroll
    for (int l = 0; l < 8; l++) rest |= v[l];
    uint8_t* mo = w.m + t * (size_t)w.np * 32;
#pragma nounroll
    for (int val = 0; val < w.np; val++) {
        u32 count = 0;
#pragma nounroll
        for (int i = 0; i < w.nd; i++) {
            const uint8_t* b = dig + (size_t)i * 32 + 28;                       // (the address depends on i alone)
            const u32 d = ((u32)b[0] << 24) | ((u32)b[1] << 16) | ((u32)b[2] << 8) | (u32)b[3];
            count += (u32)(d == (u32)val);
        }
        sc c;
        sc_set_u32(c, count);
        sc_to_be(mo + (size_t)val * 32, c);
    }
    const int32_t status = canonical ? (rest ? RW_OUT_OF_RANGE : 0) : RW_BAD_ENCODING;
    w.status[t] = status;
    return status;
}

}  // namespace bppp
