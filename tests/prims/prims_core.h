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
//
// The variable-base sums (straus_core.h) have a second record format and entry points of their own, further down: SumForm.
// The transcript primitives (merlin.h) have a third, with a program per launch, at the end: TrStep.
#pragma once
#include "../../bp_pp_amd/csrc/field.h"
#include "../../bp_pp_amd/csrc/modinv.h"
#include "../../bp_pp_amd/csrc/point.h"
#include "../../bp_pp_amd/csrc/straus_core.h"
#include "../../bp_pp_amd/csrc/draw_core.h"
#include "../../bp_pp_amd/csrc/verify_core.h"

#define PRIM_IN_WORDS 176
#define PRIM_OUT_WORDS 200
#define PRIM_BATCH_NMAX 48    // fe_batch_inv_lane: largest batch a record may describe
#define PRIM_ACC_STEPS 12     // accumulator programs: most steps a record may hold
#define PRIM_ACC_NOPROBE 0xFFu

namespace prims {
using namespace bppp;

enum Op : u32 {
    OP_FE_MUL = 1, OP_FE_SQR, OP_FE_MUL2_ADD, OP_FE_MUL_SMALL, OP_FE_ADD, OP_FE_SUB_M, OP_FE_NEG_M, OP_FE_NORMALIZE,
    OP_FE_IS_ZERO, OP_FE_IS_ODD, OP_FE_EQ, OP_FE_TO_W8, OP_FE_FROM_W8, OP_FE_INV, OP_FE_INV_FERMAT, OP_FE_SQRT, OP_FE_BATCH_INV,
    OP_SC_ADD = 32, OP_SC_SUB, OP_SC_NEG, OP_SC_MUL, OP_SC_SQR, OP_SC_REDUCE512, OP_DRAW_REDUCE512, OP_SC_INV, OP_SC_INV_FERMAT,
    OP_BE32_TO_LIMBS = 48, OP_FE_FROM_BE, OP_SC_FROM_BE, OP_SEC1_DECOMPRESS, OP_LIMBS_TO_BE32,
    OP_PT_ADD = 64, OP_PT_DBL, OP_PT_MADD_NONID, OP_PT_MADD,
    OP_GLV = 80, OP_DRAW_SCALAR,
    OP_ACCUM = 96, OP_RECODE, OP_TABLE,
};
enum AccStep : u32 { ACC_DBL = 0, ACC_MADD = 1 };
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

// ---- accumulator programs (OP_ACCUM): at most PRIM_ACC_STEPS steps over the incomplete Jacobian (kind 0: ptj_dbl, ptj_madd) or XYZZ
// (kind 1: ptz_madd) accumulator, then ptj_to_pt / ptz_to_pt.
//   in[1]       declared magnitudes of the raw start state's coordinates (X, Y, Z | X, Y, ZZ, ZZZ), one byte each
//   in[2]       kind | steps << 8 | raw start << 16 | probe step << 24 (PRIM_ACC_NOPROBE: none)
//   in[4 .. 7)  one byte per step: operand index (bits 0-1) | skip << 2 | (ACC_DBL or ACC_MADD) << 4
//   in[8 .. 88) four affine operands, x then y as 10 raw limbs each (declared magnitudes 1 and 2: a table entry whose y may be negated)
//   in[88 ..)   the raw start state (30 or 40 limbs); without it the program starts from the empty accumulator
// Out: the converted point out[0 .. 30), `empty` out[30], the raw Z (ZZ) after step s at out[31 + 10 s ..), and the whole raw accumulator
// after the probe step at out[151 ..).
HD u32 acc_step(const u32* in, u32 s) { return (in[4 + (s >> 2)] >> (8 * (s & 3))) & 0xFFu; }
HD void acc_operand(apt& q, const u32* in, u32 step) {
    const u32* w = in + 8 + 20 * (step & 3u);
    ld_fe(q.x, w, 1);
    ld_fe(q.y, w + 10, 2);
}
HD void accum_jacobian(const u32* in, u32* out, u32 ns, bool raw, u32 probe) {
    ptj a;
    bool empty = true;
    ptj_init(a);
    if (raw) {
        ld_fe(a.X, in + 88, mag_of(in, 0)); ld_fe(a.Y, in + 98, mag_of(in, 1)); ld_fe(a.Z, in + 108, mag_of(in, 2));
        empty = false;
    }
#pragma nounroll
    for (u32 s = 0; s < ns; s++) {
        const u32 b = acc_step(in, s);
        if ((b >> 4) == ACC_DBL) {
            ptj_dbl(a);
        } else {
            apt q;
            acc_operand(q, in, b);
            ptj_madd(a, empty, q, ((b >> 2) & 1u) != 0);
        }
        st_fe(out + 31 + 10 * s, a.Z);
        if (s == probe) { st_fe(out + 151, a.X); st_fe(out + 161, a.Y); st_fe(out + 171, a.Z); }
    }
    pt r;
    ptj_to_pt(r, a, empty);
    st_pt(out, r);
    out[30] = empty ? 1u : 0u;
}
HD void accum_xyzz(const u32* in, u32* out, u32 ns, bool raw, u32 probe) {
    ptz a;
    bool empty = true;
    ptz_init(a);
    if (raw) {
        ld_fe(a.X, in + 88, mag_of(in, 0)); ld_fe(a.Y, in + 98, mag_of(in, 1));
        ld_fe(a.ZZ, in + 108, mag_of(in, 2)); ld_fe(a.ZZZ, in + 118, mag_of(in, 3));
        empty = false;
    }
#pragma nounroll
    for (u32 s = 0; s < ns; s++) {
        const u32 b = acc_step(in, s);
        apt q;
        acc_operand(q, in, b);
        ptz_madd(a, empty, q, ((b >> 2) & 1u) != 0);
        st_fe(out + 31 + 10 * s, a.ZZ);
        if (s == probe) { st_fe(out + 151, a.X); st_fe(out + 161, a.Y); st_fe(out + 171, a.ZZ); st_fe(out + 181, a.ZZZ); }
    }
    pt r;
    ptz_to_pt(r, a, empty);
    st_pt(out, r);
    out[30] = empty ? 1u : 0u;
}
// ---- signed 5-bit recoding (OP_RECODE) of the 2M GLV half-scalars of an M-point sum.  in[2] = M, in[3] = 1: the M scalars at in[4 + 8 j ..)
// go through glv_decompose; in[3] = 0: glv_split contents as they stand, 12 words per point (k1[5], k2[5], neg1, neg2) at in[4 + 12 j ..).
// Out: glv_recode5's words of stream st at out[5 st ..), its 26 window digits (glv_window_digits + glv_digit_of) one byte each
// (magnitude | negative << 7) at out[50 + 7 st ..), its sign flag at out[120 + st].
template <int M>
HD void recode_case(const u32* in, u32* out, bool from_scalars) {
    glv_words<M> g;
#pragma nounroll
    for (int j = 0; j < M; j++) {
        glv_split sp;
        if (from_scalars) {
            sc k;
            ld_sc(k, in + 4 + 8 * j);
            glv_decompose(sp, k);
        } else {
            const u32* w = in + 4 + 12 * j;
#pragma unroll
            for (int i = 0; i < 5; i++) { sp.k1[i] = w[i]; sp.k2[i] = w[5 + i]; }
            sp.neg1 = (w[10] & 1u) != 0;
            sp.neg2 = (w[11] & 1u) != 0;
        }
        glv_words_set<M>(g, j, sp);
    }
#pragma nounroll
    for (int st = 0; st < 2 * M; st++) {
#pragma unroll
        for (int i = 0; i < 5; i++) out[5 * st + i] = g.w[st][i];
        out[120 + st] = g.neg[st] ? 1u : 0u;
#pragma unroll
        for (int i = 0; i < 7; i++) out[50 + 7 * st + i] = 0;
    }
#pragma nounroll
    for (int i = 0; i < BPPP_STRAUS_WINDOWS; i++) {
        const u64 pk = glv_window_digits<M>(g, i);
#pragma nounroll
        for (int st = 0; st < 2 * M; st++) {
            int mag;
            bool neg;
            glv_digit_of<M>(g, pk, st, mag, neg);
            out[50 + 7 * st + (i >> 2)] |= ((u32)mag | (neg ? 0x80u : 0u)) << (8 * (i & 3));
        }
    }
}

// ================================================================ the variable-base SUMS on tables built by the production builders
// A second record format (SUM_IN_WORDS in, SUM_OUT_WORDS out), one record per SUM of M points: the launch's configuration word
// (form | M << 8 | G << 16 | parts << 24) at in[0], point j as packed canonical words (x[8], y[8]; all zero = the identity sentinel) at
// in[4 + 16 j ..), scalar j at in[84 + 8 j ..).  Out: the sum's raw coordinates out[0 .. 30), pt_to_affine of it out[30 .. 50), out[50] =
// what the fast form returned (2: the form returns no flag), out[72] = lanes of the group whose total differs from lane 0's, out[73] = 1 when
// a lane of the group met an exceptional addition, recomputed beside the function under test (group forms).
#define SUM_IN_WORDS 128
#define SUM_OUT_WORDS 80
enum SumForm : u32 {
    SUM_AFFINE = 0,        // straus_affine<M>
    SUM_FAST_COMPLETE,     // straus_affine_fast<M>, then straus_affine_complete<M> if it returned false
    SUM_SPLIT_LANES,       // straus_split_lane<M> for the 2 M parts lanes one after the other, complete additions, fallback as straus_affine_split
    SUM_COMPLETE,          // straus_affine_complete<M> alone
    SUM_GROUP,             // straus_affine_g4<M, G> on G lanes (device only)
    SUM_SPLIT_GROUP,       // straus_affine_split<M, G, parts> on G lanes (device only)
};
HD u32 sum_cfg(u32 form, u32 m, u32 g, u32 parts) { return form | (m << 8) | (g << 16) | (parts << 24); }
// workspace of one launch of N sums, laid out as the verifiers' (limb-major / entry-major over the instances)
struct SumWs {
    size_t N;
    u32* pts;            // [16 M][N]
    u32* tscr;           // [BPPP_TSCR_PER_POINT M 10][N]
    apt_packed* atab;    // [max(parts, 1) M 16][N]
};
// tables 1P .. 16P of the record's M points by the four-inversion builder (the one-lane and lane-group sums' tables)
template <int M>
HD void sum_tables_build(const SumWs& w, size_t t, const u32* rec) {
#pragma nounroll
    for (int p = 0; p < M; p++) {
        ws_st8(w.pts, w.N, t, 2 * p, rec + 4 + 16 * p);
        ws_st8(w.pts, w.N, t, 2 * p + 1, rec + 4 + 16 * p + 8);
    }
    affine_tables_build(atab_of(w.atab, w.N, t), w.tscr, w.pts, w.N, t, M);
}
// table slot h M + p (part h of point p) by the one-lane builder (the split sums' tables, stride M between parts)
template <int M>
HD void sum_table_one(const SumWs& w, size_t t, const u32* rec, int slot, int parts) {
    const int h = slot / M, p = slot - h * M;
    apt P;
    fe_from_w8(P.x, rec + 4 + 16 * p);
    fe_from_w8(P.y, rec + 4 + 16 * p + 8);
    affine_table_one(atab_of(w.atab, w.N, t) + slot * 16, P, 5 * split_begin(parts, h));
}
template <int M>
HD void sum_scalars(glv_words<M>& g, int* pidx, const u32* rec) {
#pragma unroll
    for (int j = 0; j < M; j++) {
        sc k;
        glv_split sp;
        ld_sc(k, rec + 84 + 8 * j);
        glv_decompose(sp, k);
        glv_words_set<M>(g, j, sp);
        pidx[j] = j;
    }
}
HD void sum_outputs(u32* out, const pt& r, u32 flag) {
    st_pt(out, r);
    apt a;
    pt_to_affine(a, r);
    st_fe(out + 30, a.x);
    st_fe(out + 40, a.y);
    out[50] = flag;
}
// the forms that run on one lane
template <int M>
HD void sum_one_lane(u32 form, int parts, const SumWs& w, size_t t, const u32* rec, u32* out) {
    int pidx[M];
    glv_words<M> g;
    sum_scalars<M>(g, pidx, rec);
    const atab_ref tab = atab_of(w.atab, w.N, t);
    pt r;
    u32 flag = 2;
    if (form == SUM_AFFINE) {
        straus_affine<M>(r, tab, pidx, g);
    } else if (form == SUM_FAST_COMPLETE) {
        const bool ok = straus_affine_fast<M>(r, tab, pidx, g);
        if (!ok) straus_affine_complete<M>(r, tab, pidx, g);
        flag = ok ? 1u : 0u;
    } else if (form == SUM_COMPLETE) {
        straus_affine_complete<M>(r, tab, pidx, g);
    } else {
        bool ok = true;
        pt_set_identity(r);
#pragma nounroll
        for (int q = 0; q < 2 * M * parts; q++) {
            pt part;
            ok &= straus_split_lane<M>(part, tab, pidx, g, q, parts, M);
            pt_add(r, r, part);
        }
        if (!ok) straus_affine_complete<M>(r, tab, pidx, g);
        flag = ok ? 1u : 0u;
    }
    sum_outputs(out, r, flag);
}
HD bool sum_cfg_ok(u32 cfg) {
    const u32 form = cfg & 0xFFu, m = (cfg >> 8) & 0xFFu, g = (cfg >> 16) & 0xFFu, parts = cfg >> 24;
    if (m < 1 || m > 5) return false;
    if (form == SUM_AFFINE || form == SUM_FAST_COMPLETE || form == SUM_COMPLETE) return g == 1 && parts == 0;
    if (form == SUM_SPLIT_LANES) return g == 1 && (parts == 2 || parts == 4);
    if (form == SUM_GROUP) return (g == 2 || g == 4) && parts == 0;
    if (form == SUM_SPLIT_GROUP) return (parts == 2 || parts == 4) && (g == 8 || g == 16 || g == 32 || g == 64) && 2 * m * parts <= g;
    return false;
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
    case OP_ACCUM: {
        const u32 kind = in[2] & 0xFFu, ns = (in[2] >> 8) & 0xFFu, raw = (in[2] >> 16) & 0xFFu, probe = in[2] >> 24;
        if (kind > 1u || ns > PRIM_ACC_STEPS || raw > 1u || (probe != PRIM_ACC_NOPROBE && probe >= ns)) { st = ST_BAD_PARAM; break; }
#pragma nounroll
        for (u32 s = 0; s < ns; s++) {
            const u32 b = acc_step(in, s);
            if ((b >> 4) > ACC_MADD || (b & 8u) || (kind == 1u && (b >> 4) == ACC_DBL)) st = ST_BAD_PARAM;
        }
        if (st != ST_OK) break;
        if (kind == 0u) accum_jacobian(in, out, ns, raw != 0, probe);
        else accum_xyzz(in, out, ns, raw != 0, probe);
        break;
    }
    case OP_RECODE: {
        if (in[3] > 1u) { st = ST_BAD_PARAM; break; }
        switch (in[2]) {
        case 1: recode_case<1>(in, out, in[3] != 0); break;
        case 2: recode_case<2>(in, out, in[3] != 0); break;
        case 3: recode_case<3>(in, out, in[3] != 0); break;
        case 4: recode_case<4>(in, out, in[3] != 0); break;
        case 5: recode_case<5>(in, out, in[3] != 0); break;
        default: st = ST_BAD_PARAM;
        }
        break;
    }
    case OP_TABLE: {   // in[2] = parts | part << 8: the table of part `part` of a stream cut in `parts`; in[3] = first entry reported (1 or 9);
                       // P affine at in[4 .. 24).  Out, for the eight entries e = in[3] + k: the stored words x[8], y[8] and beta x (aff_ld,
                       // one multiplication) at out[24 k ..); out[192] = the doublings done first, out[193] = entries aff_ld did not return as stored
        const u32 parts = in[2] & 0xFFu, part = (in[2] >> 8) & 0xFFu;
        if ((parts != 1u && parts != 2u && parts != 4u && parts != 8u) || part >= parts || (in[2] >> 16) || (in[3] != 1u && in[3] != 9u)) {
            st = ST_BAD_PARAM;
            break;
        }
        apt P;
        ld_fe(P.x, x, 1); ld_fe(P.y, x + 10, 1);
        apt_packed tab[16];
        const atab_ref tb = {tab, 1};
        const int pre = 5 * split_begin((int)parts, (int)part);
        affine_table_one(tb, P, pre);
        fe beta;
        glv_beta(beta);
        u32 differ = 0;
#pragma nounroll
        for (int k = 0; k < 8; k++) {
            const int e = (int)in[3] + k;
            aff_src a;
            aff_ld(a, tb, e);
            u32 back[8];
            fe bx;
            u32* o = out + 24 * k;
#pragma unroll
            for (int i = 0; i < 8; i++) { o[i] = tab[e - 1].x[i]; o[8 + i] = tab[e - 1].y[i]; }
            fe_to_w8(back, a.x);
#pragma unroll
            for (int i = 0; i < 8; i++) differ |= back[i] ^ o[i];
            fe_to_w8(back, a.y);
#pragma unroll
            for (int i = 0; i < 8; i++) differ |= back[i] ^ o[8 + i];
            fe_mul(bx, a.x, beta);
            fe_to_w8(o + 16, bx);
        }
        out[192] = (u32)pre;
        out[193] = differ ? 1u : 0u;
        break;
    }
    default:
        st = ST_BAD_OP;
    }
    out[PRIM_OUT_WORDS - 1] = st;
}

// ================================================================ the TRANSCRIPT primitives (merlin.h, verify_ws.h: app_point, the 203-byte state)
// A third record format and entry points of its own: one launch runs ONE program of at most TR_MAX_STEPS steps over n records, because the
// sponge's byte position has to be uniform over a wavefront (merlin.h: st_uniform) and the launch layout is therefore part of the test.
//   program   TR_PROG_WORDS words: the number of steps, then (kind, label id, parameter) per step
//   states    n x 203 bytes, the layout of strobe_from_bytes / strobe_to_bytes
//   record    TR_IN_WORDS words: in[0 .. 64) 256 message bytes | in[64 .. 144) four affine points, x then y as 10 canonical limbs each
//             (all zero: the identity) | in[144 .. 148) two u64 (low word first) | in[148 .. 150) the u64 of TS_ROTL64 | in[150] the word of
//             TS_ABSORB_CHUNK
//   output    TR_OUT_WORDS words: out[0 .. 51) the 203 state bytes after the program (strobe_to_bytes; byte 202 = the flags of the last
//             operation begun, the input's where the program begins none) | out[51] status | out[52 ..) what the steps produced, one after
//             the other: squeezed bytes packed little-endian into whole words, a challenge as its 8 words and the canonical flag
// A state strobe_from_bytes refuses is answered with TR_BAD_STATE and not evaluated; a program that breaks a bound with ST_BAD_PARAM.
#define TR_MAX_STEPS 8
#define TR_PROG_WORDS (1 + 3 * TR_MAX_STEPS)
#define TR_IN_WORDS 152
#define TR_PROD_WORDS 128
#define TR_OUT_WORDS (52 + TR_PROD_WORDS)
#define TR_MSG_BYTES 256
enum TrStep : u32 {
    // raw steps
    TS_KECCAK_F = 1,       // keccak_f1600 on the 25 state words
    TS_KECCAK_RC,          // keccak_rc(par), par < 24: 2 words
    TS_ROTL64,             // rotl64(v, par), 1 <= par <= 63: 2 words
    TS_ABSORB_CHUNK,       // strobe_absorb_chunk(word, par), 1 <= par <= 4
    TS_RUN_F,              // strobe_run_f
    TS_SQUEEZE,            // strobe_squeeze of par <= 200 bytes
    TS_META_AD,            // strobe_meta_ad / strobe_ad of the first (par & 0xFFFF) <= 256 message bytes, `more` = par >> 16 (register sponge)
    TS_AD,
    TS_PRF,                // strobe_prf of par <= 200 bytes (register sponge)
    // transcript steps (label id: TR_LABELS_*)
    TS_APPEND_MEM = 16,    // t_append of the first par <= 200 message bytes (register sponge)
    TS_APPEND_WORDS,       // t_append_words<NW = 9> of the first 9 message words, par <= 36 bytes
    TS_APPEND_U64,         // t_append_u64 of u64 number par < 2
    TS_APP_POINT,          // app_point of point number par < 4
    TS_GET_CHALLENGE,      // t_get_challenge: 9 words
    TS_CHALLENGE_BYTES,    // t_challenge_bytes of par <= 200 bytes; LDS sponge: the same challenge header (t_op_absorb), then strobe_squeeze
};
enum TrForm : u32 { TR_REGS = 0, TR_LDS = 1 };                     // strobe | strobe_lds (device only)
enum TrLayout : u32 { TR_UNIFORM = 0, TR_GROUPED = 1 };            // device: body called directly | inside for_each_position_group
enum TrStatus : u32 { TR_BAD_STATE = 4, TR_BAD_LAYOUT = 5 };       // beside Status
// Labels are compile-time arrays: a fixed list, by id.  ANY: every transcript step takes them (the product's short labels and test labels of
// length 1, 2, 3, 5, 6, so that L mod 4 takes every value); POINT: app_point only; CHAL: t_get_challenge only (the rest of the labels that the
// protocols' longest sequences use).
#define TR_LABELS_ANY(X) X(0, "dom-sep") X(1, "l.sz") X(2, "n.sz") X(3, "wnla_challenge") X(4, "circuit_rho") X(5, "reciprocal_challenge") \
    X(6, "a") X(7, "bc") X(8, "def") X(9, "ghijk") X(10, "lmnopq")
#define TR_LABELS_POINT(X) X(11, "wnla_com") X(12, "wnla_x") X(13, "wnla_r") X(14, "reciprocal_commitment") X(15, "commitment_cl") \
    X(16, "commitment_cr") X(17, "commitment_co") X(18, "commitment_v") X(19, "commitment_cs")
#define TR_LABELS_CHAL(X) X(20, "circuit_lambda") X(21, "circuit_beta") X(22, "circuit_delta") X(23, "circuit_tau")
#define TR_N_ANY 11
#define TR_N_POINT 20
#define TR_N_LABELS 24
// calls f(label) with label number `lab` as the literal itself; CLS bit 0: the POINT labels too, bit 1: the CHAL labels too
template <int CLS, typename F>
HD void tr_with_label(u32 lab, F&& f) {
    switch (lab) {
#define TR_X(i, s) case i: f(s); break;
        TR_LABELS_ANY(TR_X)
#undef TR_X
    default:
        if constexpr ((CLS & 1) != 0) {
            switch (lab) {
#define TR_X(i, s) case i: f(s); break;
                TR_LABELS_POINT(TR_X)
#undef TR_X
            default: break;
            }
        }
        if constexpr ((CLS & 2) != 0) {
            switch (lab) {
#define TR_X(i, s) case i: f(s); break;
                TR_LABELS_CHAL(TR_X)
#undef TR_X
            default: break;
            }
        }
    }
}
HD bool tr_label_ok(u32 kind, u32 lab) {
    if (lab < TR_N_ANY) return true;
    if (lab < TR_N_POINT) return kind == TS_APP_POINT;
    return lab < TR_N_LABELS && kind == TS_GET_CHALLENGE;
}
// words a step appends to the record's products
HD u32 tr_step_words(u32 kind, u32 par) {
    switch (kind) {
    case TS_KECCAK_RC: case TS_ROTL64: return 2;
    case TS_SQUEEZE: case TS_PRF: case TS_CHALLENGE_BYTES: return (par + 3) / 4;
    case TS_GET_CHALLENGE: return 9;
    default: return 0;
    }
}
// the bounds of a program, for the sponge form that is to run it
HD bool tr_prog_ok(const u32* prog, u32 form) {
    const u32 ns = prog[0];
    if (ns > TR_MAX_STEPS || form > TR_LDS) return false;
    u32 words = 0;
#pragma nounroll
    for (u32 s = 0; s < ns; s++) {
        const u32 kind = prog[1 + 3 * s], lab = prog[2 + 3 * s], par = prog[3 + 3 * s];
        bool ok;
        switch (kind) {
        case TS_KECCAK_F: case TS_RUN_F: ok = par == 0; break;
        case TS_KECCAK_RC: ok = par < 24; break;
        case TS_ROTL64: ok = par >= 1 && par <= 63; break;
        case TS_ABSORB_CHUNK: ok = par >= 1 && par <= 4; break;
        case TS_SQUEEZE: ok = par <= 200; break;
        case TS_META_AD: case TS_AD: ok = form == TR_REGS && (par & 0xFFFFu) <= TR_MSG_BYTES && (par >> 16) <= 1; break;
        case TS_PRF: ok = form == TR_REGS && par <= 200; break;
        case TS_APPEND_MEM: ok = form == TR_REGS && par <= 200; break;
        case TS_APPEND_WORDS: ok = par <= 36; break;
        case TS_APPEND_U64: ok = par < 2; break;
        case TS_APP_POINT: ok = par < 4; break;
        case TS_GET_CHALLENGE: ok = par == 0; break;
        case TS_CHALLENGE_BYTES: ok = par <= 200; break;
        default: ok = false;
        }
        if (kind < TS_APPEND_MEM) ok = ok && lab == 0;
        else ok = ok && tr_label_ok(kind, lab);
        if (!ok) return false;
        words += tr_step_words(kind, par);
    }
    return words <= TR_PROD_WORDS;
}
HD u64 tr_rotl64(u64 v, u32 r) {     // rotl64 takes a compile-time amount: one call per amount
    u64 o = v;
    switch (r) {
#define TR_R(i) case i: o = rotl64(v, i); break;
#define TR_R8(b) TR_R(b) TR_R(b + 1) TR_R(b + 2) TR_R(b + 3) TR_R(b + 4) TR_R(b + 5) TR_R(b + 6) TR_R(b + 7)
        TR_R(1) TR_R(2) TR_R(3) TR_R(4) TR_R(5) TR_R(6) TR_R(7)
        TR_R8(8) TR_R8(16) TR_R8(24) TR_R8(32) TR_R8(40) TR_R8(48) TR_R8(56)
#undef TR_R8
#undef TR_R
    default: break;
    }
    return o;
}
HD void tr_keccak_f(strobe& s) { keccak_f1600(s.st); }
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void tr_keccak_f(strobe_lds& s) { keccak_f1600_lds(s.col); }
#endif
// the steps only the register sponge has (memory operands, strobe& signatures)
HD void tr_step_regs(strobe& t, u32 kind, u32 lab, u32 par, const uint8_t* msg, u32* prod, u32& flags) {
    uint8_t buf[200];
    if (kind == TS_META_AD) { strobe_meta_ad(t, msg, par & 0xFFFFu, (par >> 16) != 0); if (!(par >> 16)) flags = 16 | 2; }
    else if (kind == TS_AD) { strobe_ad(t, msg, par & 0xFFFFu, (par >> 16) != 0); if (!(par >> 16)) flags = 2; }
    else if (kind == TS_PRF) {
#pragma nounroll
        for (u32 i = 0; i < 200; i++) buf[i] = 0;
        strobe_prf(t, buf, par);
        st_bytes(prod, buf, (int)par);
        flags = 1 | 2 | 4;
    } else if (kind == TS_APPEND_MEM) {
        tr_with_label<0>(lab, [&](const auto& label) { t_append(t, label, msg, par); });
        flags = 2;
    } else {     // TS_CHALLENGE_BYTES
#pragma nounroll
        for (u32 i = 0; i < 200; i++) buf[i] = 0;
        tr_with_label<0>(lab, [&](const auto& label) { t_challenge_bytes(t, label, buf, par); });
        st_bytes(prod, buf, (int)par);
        flags = 1 | 2 | 4;
    }
}
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void tr_step_regs(strobe_lds& t, u32 kind, u32 lab, u32 par, const uint8_t*, u32* prod, u32& flags) {
    if (kind != TS_CHALLENGE_BYTES) return;     // tr_prog_ok lets nothing else through
    uint8_t buf[200];
#pragma nounroll
    for (u32 i = 0; i < 200; i++) buf[i] = 0;
    tr_with_label<0>(lab, [&](const auto& label) { t_op_absorb(t, label, par, 1, [](u32) -> u32 { return 0; }); });
    strobe_squeeze(t, buf, par);
    st_bytes(prod, buf, (int)par);
    flags = 1 | 2 | 4;
}
#endif
// One step on either sponge form.  `prod` is where the step's products go.
template <typename S>
HD void tr_step(S& t, u32 kind, u32 lab, u32 par, const u32* rec, u32* prod, u32& flags) {
    switch (kind) {
    case TS_KECCAK_F: tr_keccak_f(t); break;
    case TS_KECCAK_RC: { const u64 c = keccak_rc((int)par); prod[0] = (u32)c; prod[1] = (u32)(c >> 32); break; }
    case TS_ROTL64: {
        const u64 o = tr_rotl64((u64)rec[148] | ((u64)rec[149] << 32), par);
        prod[0] = (u32)o; prod[1] = (u32)(o >> 32);
        break;
    }
    case TS_ABSORB_CHUNK: {
        const u32 mask = par >= 4 ? 0xFFFFFFFFu : ((1u << (8 * par)) - 1u);     // the contract: unused high bytes zero
        strobe_absorb_chunk(t, rec[150] & mask, par);
        break;
    }
    case TS_RUN_F: strobe_run_f(t); break;
    case TS_SQUEEZE: {
        uint8_t buf[200];
#pragma nounroll
        for (u32 i = 0; i < 200; i++) buf[i] = 0;
        strobe_squeeze(t, buf, par);
        st_bytes(prod, buf, (int)par);
        break;
    }
    case TS_APPEND_WORDS: {
        u32 mw[9];
#pragma unroll
        for (int k = 0; k < 9; k++) mw[k] = rec[k];
        tr_with_label<0>(lab, [&](const auto& label) { t_append_words(t, label, mw, par); });
        flags = 2;
        break;
    }
    case TS_APPEND_U64: {
        const u64 x = (u64)rec[144 + 2 * par] | ((u64)rec[145 + 2 * par] << 32);
        tr_with_label<0>(lab, [&](const auto& label) { t_append_u64(t, label, x); });
        flags = 2;
        break;
    }
    case TS_APP_POINT: {
        apt a;
        ld_fe(a.x, rec + 64 + 20 * par, 1);
        ld_fe(a.y, rec + 74 + 20 * par, 1);
        tr_with_label<1>(lab, [&](const auto& label) { app_point(t, label, a); });
        flags = 2;
        break;
    }
    case TS_GET_CHALLENGE: {
        sc c;
        bool ok = false;
        sc_set_u32(c, 0);
        tr_with_label<2>(lab, [&](const auto& label) { ok = t_get_challenge(t, label, c); });
        st_sc(prod, c);
        prod[8] = ok ? 1u : 0u;
        flags = 1 | 2 | 4;
        break;
    }
    default: tr_step_regs(t, kind, lab, par, (const uint8_t*)rec, prod, flags); break;
    }
}
// the program over one sponge that is loaded already; returns the flags of the last operation begun
template <typename S>
HD u32 tr_run_program(S& t, const u32* prog, const u32* rec, u32* out, u32 flags) {
    u32 cur = 52;
#pragma nounroll
    for (u32 s = 0; s < prog[0]; s++) {
        const u32 kind = prog[1 + 3 * s], lab = prog[2 + 3 * s], par = prog[3 + 3 * s];
        tr_step(t, kind, lab, par, rec, out + cur, flags);
        cur += tr_step_words(kind, par);
    }
    return flags;
}
// One record on the register sponge (every build).  The caller has checked the program (tr_prog_ok).
HD void tr_eval_regs(const u32* prog, const uint8_t* state, const u32* rec, u32* out) {
    strobe t;
    if (!strobe_from_bytes(t, state)) { out[51] = TR_BAD_STATE; return; }
    const u32 flags = tr_run_program(t, prog, rec, out, state[202]);
    uint8_t b[204];
    b[203] = 0;
    strobe_to_bytes(b, t, flags);
    st_bytes(out, b, 204);
    out[51] = ST_OK;
}

}  // namespace prims
