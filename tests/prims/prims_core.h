// TEST-ONLY case dispatcher over the field, scalar and group primitives, compiled three ways from this one file: g++ and clang++ for
// the host (prims_host.cpp), hipcc --offload-arch=gfx950 for the device (prims_device.hip).  One record = PRIM_IN_WORDS input words
// and PRIM_OUT_WORDS output words; tests/test_prims.py builds the records and checks the outputs against big integers.
//
// Input record:  in[0] op code | in[1] declared magnitudes of the field operands, one byte each (operand 0 in the low byte)
//                in[2], in[3]  op parameters (see each case) | in[4 ..] operands, field elements as 10 raw limbs, scalars as 8 words
// Output record: out[0 ..] results | out[PRIM_OUT_WORDS - 1] status (0 = evaluated, else the record broke the dispatcher's rules)
//
// Field elements are loaded and stored limb by limb (never by struct copy); the host build sets each operand's declared magnitude,
// so the FE_CHECK asserts of field.h guard the contract of every call.  The device build carries no magnitude.
#pragma once
#include "../../bp_pp_amd/csrc/field.h"
#include "../../bp_pp_amd/csrc/modinv.h"
#include "../../bp_pp_amd/csrc/point.h"
#include "../../bp_pp_amd/csrc/straus_core.h"
#include "../../bp_pp_amd/csrc/draw_core.h"
#include "../../bp_pp_amd/csrc/verify_core.h"

#define PRIM_IN_WORDS 176
#define PRIM_OUT_WORDS 168
#define PRIM_BATCH_NMAX 48    // fe_batch_inv_lane: largest batch a record may describe

namespace prims {
using namespace bppp;

enum Op : u32 {
    OP_FE_MUL = 1, OP_FE_SQR, OP_FE_MUL2_ADD, OP_FE_MUL_SMALL, OP_FE_ADD, OP_FE_SUB_M, OP_FE_NEG_M, OP_FE_NORMALIZE,
    OP_FE_IS_ZERO, OP_FE_IS_ODD, OP_FE_EQ, OP_FE_TO_W8, OP_FE_FROM_W8, OP_FE_INV, OP_FE_INV_FERMAT, OP_FE_SQRT, OP_FE_BATCH_INV,
    OP_SC_ADD = 32, OP_SC_SUB, OP_SC_NEG, OP_SC_MUL, OP_SC_SQR, OP_SC_REDUCE512, OP_DRAW_REDUCE512, OP_SC_INV, OP_SC_INV_FERMAT,
    OP_BE32_TO_LIMBS = 48, OP_FE_FROM_BE, OP_SC_FROM_BE, OP_SEC1_DECOMPRESS, OP_LIMBS_TO_BE32,
    OP_PT_ADD = 64, OP_PT_DBL, OP_PT_MADD_NONID, OP_PT_MADD,
    OP_GLV = 80, OP_DRAW_SCALAR,
};
enum Status : u32 { ST_OK = 0, ST_BAD_OP = 1, ST_BAD_PARAM = 2, ST_BAD_OFFSET = 3 };

HD int mag_of(const u32* in, int k) { return (int)((in[1] >> (8 * k)) & 0xFFu); }
HD void ld_fe(fe& a, const u32* w, int mag) {
#pragma unroll
    for (int i = 0; i < 10; i++) a.v[i] = w[i];
    FE_SETMAG(a, mag);
    (void)mag;
}
HD void st_fe(u32* w, const fe& a) {
#pragma unroll
    for (int i = 0; i < 10; i++) w[i] = a.v[i];
}
HD void ld_sc(sc& a, const u32* w) {
#pragma unroll
    for (int i = 0; i < 8; i++) a.v[i] = w[i];
}
HD void st_sc(u32* w, const sc& a) {
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = a.v[i];
}
// magnitudes of the three coordinates in one word, one byte each
HD void ld_pt(pt& p, const u32* w, u32 mags) {
    ld_fe(p.X, w, (int)(mags & 0xFFu));
    ld_fe(p.Y, w + 10, (int)((mags >> 8) & 0xFFu));
    ld_fe(p.Z, w + 20, (int)((mags >> 16) & 0xFFu));
}
HD void st_pt(u32* w, const pt& p) {
    st_fe(w, p.X);
    st_fe(w + 10, p.Y);
    st_fe(w + 20, p.Z);
}
// bytes -> words, little-endian within a word (byte k of the output lands in bits 8 (k % 4) of word k / 4)
HD void st_bytes(u32* w, const uint8_t* b, int n) {
#pragma nounroll
    for (int k = 0; k < n; k += 4) w[k / 4] = (u32)b[k] | ((u32)b[k + 1] << 8) | ((u32)b[k + 2] << 16) | ((u32)b[k + 3] << 24);
}

// a group operation's result: raw coordinates (out[0 .. 30)), pt_to_affine of it (out[30 .. 50)), pt_eq against the canonical
// projective point at in[64 .. 94) (out[50])
HD void pt_outputs(u32* out, const pt& r, const u32* in) {
    st_pt(out, r);
    apt a;
    pt_to_affine(a, r);
    st_fe(out + 30, a.x);
    st_fe(out + 40, a.y);
    pt e;
    ld_pt(e, in + 64, 0x010101u);
    out[50] = pt_eq(r, e) ? 1u : 0u;
}

// fe_batch_inv_lane<G> for lane i of a batch of N: the record holds the G elements the lane takes (t = i + j L, L = ceil(N / G),
// slots with t >= N unused), each at in[4 + 10 j].  Out: the lane's results at out[10 j], and out[160] = the number of batch words
// outside the lane's own elements that the call changed (must be 0).  in[3] bit 16: in place (in == out, as the product allows).
template <int G>
HD void batch_inv_case(const u32* in, u32* out, u32 n, u32 i, bool in_place) {
    u32 a[10 * PRIM_BATCH_NMAX], b[10 * PRIM_BATCH_NMAX];
    const u32 L = (n + G - 1) / G;
#pragma nounroll
    for (u32 k = 0; k < 10 * n; k++) { a[k] = 0x5A5A5A5Au; b[k] = 0xA5A5A5A5u; }
#pragma nounroll
    for (int j = 0; j < G; j++) {
        const u32 t = i + (u32)j * L;
        if (t < n) {
#pragma nounroll
            for (int k = 0; k < 10; k++) a[k * n + t] = in[4 + 10 * j + k];
        }
    }
    u32* dst = in_place ? a : b;
    fe_batch_inv_lane<G>(a, dst, n, i);
    u32 foreign = 0;
#pragma nounroll
    for (u32 t = 0; t < n; t++) {
        const bool mine = t >= i && (t - i) % L == 0 && (t - i) / L < (u32)G;
#pragma nounroll
        for (int k = 0; k < 10; k++) {
            const u32 w = dst[k * n + t];
            if (mine) out[10 * ((t - i) / L) + k] = w;
            else foreign += (w != (in_place ? 0x5A5A5A5Au : 0xA5A5A5A5u)) ? 1u : 0u;
        }
    }
    out[160] = foreign;
}

// Evaluates one record.  `bytes` (nbytes long) is the byte-buffer side input of the byte ops, read at offset in[2].
HD void prim_eval(u32 op, const u32* in, u32* out, const uint8_t* bytes, size_t nbytes) {
    u32 st = ST_OK;
    const u32* x = in + 4;
    switch (op) {
    case OP_FE_MUL: {
        fe a, b, r;
        ld_fe(a, x, mag_of(in, 0)); ld_fe(b, x + 10, mag_of(in, 1));
        fe_mul(r, a, b);
        st_fe(out, r);
        break;
    }
    case OP_FE_SQR: {
        fe a, r;
        ld_fe(a, x, mag_of(in, 0));
        fe_sqr(r, a);
        st_fe(out, r);
        break;
    }
    case OP_FE_MUL2_ADD: {
        fe a, b, c, d, r;
        ld_fe(a, x, mag_of(in, 0)); ld_fe(b, x + 10, mag_of(in, 1)); ld_fe(c, x + 20, mag_of(in, 2)); ld_fe(d, x + 30, mag_of(in, 3));
        fe_mul2_add(r, a, b, c, d);
        st_fe(out, r);
        break;
    }
    case OP_FE_MUL_SMALL: {
        fe a, r;
        ld_fe(a, x, mag_of(in, 0));
        if (in[2] > 32u) { st = ST_BAD_PARAM; break; }
        fe_mul_small(r, a, in[2]);
        st_fe(out, r);
        break;
    }
    case OP_FE_ADD: {
        fe a, b, r;
        ld_fe(a, x, mag_of(in, 0)); ld_fe(b, x + 10, mag_of(in, 1));
        fe_add(r, a, b);
        st_fe(out, r);
        break;
    }
    case OP_FE_SUB_M: {   // in[2] = M
        fe a, b, r;
        ld_fe(a, x, mag_of(in, 0)); ld_fe(b, x + 10, mag_of(in, 1));
        switch (in[2]) {
        case 1: fe_sub_m<1>(r, a, b); break;
        case 2: fe_sub_m<2>(r, a, b); break;
        case 3: fe_sub_m<3>(r, a, b); break;
        case 4: fe_sub_m<4>(r, a, b); break;
        case 5: fe_sub_m<5>(r, a, b); break;
        case 6: fe_sub_m<6>(r, a, b); break;
        default: st = ST_BAD_PARAM;
        }
        if (st == ST_OK) st_fe(out, r);
        break;
    }
    case OP_FE_NEG_M: {   // in[2] = M
        fe a, r;
        ld_fe(a, x, mag_of(in, 0));
        if (in[2] == 1) fe_neg_m<1>(r, a);
        else if (in[2] == 3) fe_neg_m<3>(r, a);
        else { st = ST_BAD_PARAM; break; }
        st_fe(out, r);
        break;
    }
    case OP_FE_NORMALIZE: {
        fe a;
        ld_fe(a, x, mag_of(in, 0));
        fe_normalize(a);
        st_fe(out, a);
        break;
    }
    case OP_FE_IS_ZERO: {
        fe a;
        ld_fe(a, x, mag_of(in, 0));
        out[0] = fe_is_zero(a) ? 1u : 0u;
        break;
    }
    case OP_FE_IS_ODD: {
        fe a;
        ld_fe(a, x, mag_of(in, 0));
        out[0] = fe_is_odd(a) ? 1u : 0u;
        break;
    }
    case OP_FE_EQ: {
        fe a, b;
        ld_fe(a, x, mag_of(in, 0)); ld_fe(b, x + 10, mag_of(in, 1));
        out[0] = fe_eq(a, b) ? 1u : 0u;
        break;
    }
    case OP_FE_TO_W8: {   // out[0 .. 8) = fe_to_w8(a), out[8 .. 18) = fe_from_w8 of those words
        fe a, r;
        u32 w[8];
        ld_fe(a, x, mag_of(in, 0));
        fe_to_w8(w, a);
        fe_from_w8(r, w);
#pragma unroll
        for (int i = 0; i < 8; i++) out[i] = w[i];
        st_fe(out + 8, r);
        break;
    }
    case OP_FE_FROM_W8: {   // any 8 words: out[0 .. 10) = fe_from_w8, out[10 .. 18) = fe_to_w8 of that
        fe r;
        u32 w[8];
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = x[i];
        fe_from_w8(r, w);
        st_fe(out, r);
        fe_to_w8(out + 10, r);
        break;
    }
    case OP_FE_INV: {
        fe a, r;
        ld_fe(a, x, mag_of(in, 0));
        fe_inv(r, a);
        st_fe(out, r);
        break;
    }
    case OP_FE_INV_FERMAT: {
        fe a, r;
        ld_fe(a, x, mag_of(in, 0));
        fe_inv_fermat(r, a);
        st_fe(out, r);
        break;
    }
    case OP_FE_SQRT: {
        fe a, r;
        ld_fe(a, x, mag_of(in, 0));
        fe_sqrt_candidate(r, a);
        st_fe(out, r);
        break;
    }
    case OP_FE_BATCH_INV: {   // in[2] = G, in[3] = N | i << 8 | in_place << 16
        const u32 g = in[2], n = in[3] & 0xFFu, i = (in[3] >> 8) & 0xFFu;
        const bool in_place = ((in[3] >> 16) & 1u) != 0;
        if (n == 0 || n > PRIM_BATCH_NMAX || g * 10u + 4u > PRIM_IN_WORDS || i >= (n + g - 1) / g) { st = ST_BAD_PARAM; break; }
        if (g == 2) batch_inv_case<2>(in, out, n, i, in_place);
        else if (g == 4) batch_inv_case<4>(in, out, n, i, in_place);
        else if (g == 8) batch_inv_case<8>(in, out, n, i, in_place);
        else if (g == 16) batch_inv_case<16>(in, out, n, i, in_place);
        else st = ST_BAD_PARAM;
        break;
    }
    case OP_SC_ADD: case OP_SC_SUB: case OP_SC_MUL: {
        sc a, b, r;
        ld_sc(a, x); ld_sc(b, x + 8);
        if (op == OP_SC_ADD) sc_add(r, a, b);
        else if (op == OP_SC_SUB) sc_sub(r, a, b);
        else sc_mul(r, a, b);
        st_sc(out, r);
        break;
    }
    case OP_SC_NEG: case OP_SC_SQR: case OP_SC_INV: case OP_SC_INV_FERMAT: {
        sc a, r;
        ld_sc(a, x);
        if (op == OP_SC_NEG) sc_neg(r, a);
        else if (op == OP_SC_SQR) sc_sqr(r, a);
        else if (op == OP_SC_INV) sc_inv(r, a);
        else sc_inv_fermat(r, a);
        st_sc(out, r);
        break;
    }
    case OP_SC_REDUCE512: {
        sc r;
        sc_reduce512(r, x);
        st_sc(out, r);
        break;
    }
    case OP_DRAW_REDUCE512: {
        draw_reduce512(out, x);
        break;
    }
    case OP_BE32_TO_LIMBS: case OP_FE_FROM_BE: case OP_SC_FROM_BE: case OP_SEC1_DECOMPRESS: {   // in[2] = byte offset
        const size_t off = in[2], len = op == OP_SEC1_DECOMPRESS ? 33 : 32;
        if (off > nbytes || nbytes - off < len) { st = ST_BAD_OFFSET; break; }
        const uint8_t* b = bytes + off;
        if (op == OP_BE32_TO_LIMBS) be32_to_limbs(out, b);
        else if (op == OP_FE_FROM_BE) {
            fe r;
            const bool ok = fe_from_be(r, b);
            st_fe(out, r);
            out[10] = ok ? 1u : 0u;
        } else if (op == OP_SC_FROM_BE) {
            sc r;
            const bool ok = sc_from_be(r, b);
            st_sc(out, r);
            out[8] = ok ? 1u : 0u;
        } else {   // in[3] = offset of the 64-byte output in a 16-byte aligned scratch buffer
            if (in[3] > 15u) { st = ST_BAD_PARAM; break; }
            alignas(16) uint8_t buf[80];
            sec1_decompress_to_xy64(buf + in[3], b);
            st_bytes(out, buf + in[3], 64);
        }
        break;
    }
    case OP_LIMBS_TO_BE32: {   // in[3] = offset of the 32-byte output in a 16-byte aligned scratch buffer
        if (in[3] > 15u) { st = ST_BAD_PARAM; break; }
        alignas(16) uint8_t buf[48];
        limbs_to_be32(buf + in[3], x);
        st_bytes(out, buf + in[3], 32);
        break;
    }
    case OP_PT_ADD: case OP_PT_DBL: {   // p at in[4 .. 34) (magnitudes in[1]), q at in[34 .. 64) (magnitudes in[2])
        pt p, r;
        ld_pt(p, x, in[1]);
        if (op == OP_PT_ADD) {
            pt q;
            ld_pt(q, x + 30, in[2]);
            pt_add(r, p, q);
        } else {
            pt_dbl(r, p);
        }
        pt_outputs(out, r, in);
        break;
    }
    case OP_PT_MADD_NONID: case OP_PT_MADD: {   // q affine at in[34 .. 54) (magnitudes in[2]); in[3] = skip (pt_madd)
        pt p, r;
        apt q;
        ld_pt(p, x, in[1]);
        ld_fe(q.x, x + 30, (int)(in[2] & 0xFFu));
        ld_fe(q.y, x + 40, (int)((in[2] >> 8) & 0xFFu));
        if (op == OP_PT_MADD_NONID) pt_madd_nonid(r, p, q);
        else pt_madd(r, p, q, in[3] != 0);
        pt_outputs(out, r, in);
        break;
    }
    case OP_GLV: {   // out[0 .. 5) k1, [5 .. 10) k2, [10] neg1, [11] neg2
        sc k;
        glv_split s;
        ld_sc(k, x);
        glv_decompose(s, k);
#pragma unroll
        for (int i = 0; i < 5; i++) { out[i] = s.k1[i]; out[5 + i] = s.k2[i]; }
        out[10] = s.neg1 ? 1u : 0u;
        out[11] = s.neg2 ? 1u : 0u;
        break;
    }
    case OP_DRAW_SCALAR: {   // key at in[4 .. 12), stream in[12 .. 14), counter in[14 .. 16) (low word first)
        const u64 stream = (u64)x[8] | ((u64)x[9] << 32), counter = (u64)x[10] | ((u64)x[11] << 32);
        draw_scalar_words(out, x, stream, counter);
        break;
    }
    default:
        st = ST_BAD_OP;
    }
    out[PRIM_OUT_WORDS - 1] = st;
}

}  // namespace prims
