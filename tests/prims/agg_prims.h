// TEST-ONLY: what the two builds of the aggregate-stage entry points share (prims_host.cpp: prims_run_agg_verify_host /
// prims_run_agg_prove_host, the single-thread form of agg_core.h / agg_prove_core.h as tests/emul runs it; agg_device.hip:
// prims_run_agg_verify_device / prims_run_agg_prove_device, the product's k_agg_* / k_aprove_* kernels).  tests/test_prims_agg.py calls
// both with plain arrays and compares every buffer with the Python oracle.
//
// Verifier:  dims[AGGV_NDIMS] = N, k, nd, np, rounds, nl, nn, NG, NH, form, W, label_len
//            in[4]            = label | fixed-base table of the 1 + NG + NH bases g | g_vec||g_vec_ | h_vec||h_vec_ (prims_bucket_fb_build)
//                               | commitments N x k x 64 | proofs N x proof_bytes
//            io[AGGV_NBUFS]   = the workspace buffers of AggWs in the kernels' own layout ([word][N] for the word arrays), handed in
//                               pre-filled (the caller's sentinel) and handed back as the stages left them; the last one, `fell`, one byte
//                               per instance: bit c set when chunk c of the variable-base sum met an exceptional addition
//                               (straus_affine_fast recomputed beside the sum; 0 on the projective-table form)
//   form: bits 0-3 lanes per instance of phase 1 (1: k_agg_phase1; 2, 4, 8: k_agg_phase1_grp) | bits 4-7 the fixed-base kernel
//         (AGGV_FB_*) | bit 8 set: window tables (k_agg_c0_tables, atab), clear: atab = nullptr, the projective-table Straus on w.straus
// Prover:    dims[AGGP_NDIMS] = N, k, nd, np, NG, NH, stages, label_len
//            in[2]            = label | the fixed-base table (as the verifier's; read by the msm stage only, may be null without it)
//            io[AGGP_NBUFS]   = every buffer of AggProveWs the four stages read or write; a stage's inputs are what the caller (or the
//                               stage before it) left there.  stages: AGGP_WITNESS | AGGP_R1 | AGGP_MSM | AGGP_R2, run in that order
//                               (the order of agg_prove_part); AGGP_CT: ct = 1 in k_aprove_msm (the constant-time lookups over the
//                               same 4-bit table, as ensure_ct_table hands it over when the context's own table has that width)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../bp_pp_amd/csrc/agg_prove_core.h"

#define AGGV_NDIMS 12
#define AGGV_NBUFS 13
#define AGGV_FB_L1 0
#define AGGV_FB_LANES 1
#define AGGV_FB_L64 2
#define AGGV_FORM_TABLES 0x100u
#define AGGP_NDIMS 8
#define AGGP_NBUFS 20
#define AGGP_WITNESS 1
#define AGGP_R1 2
#define AGGP_MSM 4
#define AGGP_R2 8
#define AGGP_CT 16
#define AGG_MAX_N 4096

namespace aggp {

enum VBuf { V_STATUS, V_TSTATE, V_SC0, V_PTS, V_ACC, V_PFIX, V_INV, V_VSUM, V_COMMIT, V_C, V_RHO, V_MU, V_FELL };
enum PBuf { P_X, P_S, P_RND, P_COM, P_DIGITS, P_M, P_STATUS, P_ROW_STATUS, P_VSC, P_TSTATE, P_INST, P_SCR, P_RSC, P_RPB, P_VSUM, P_CP_V,
            P_CP_SV, P_CP_WR, P_CP_VPTS, P_PROOF_R };
static_assert(V_FELL + 1 == AGGV_NBUFS && P_PROOF_R + 1 == AGGP_NBUFS, "buffer counts");

struct VerifyShape {
    size_t N, k, nd, np, rounds, nl, nn, NG, NH, W, label_len, proof_bytes;
    uint32_t form;
    int G, fb;
    bool tables;
};
// the bounds of agg_shape_check (bppp_generic.hip) and of this launcher: every index the kernels form stays inside a buffer
inline bool verify_shape(VerifyShape& s, const int64_t* d) {
    for (int i = 0; i < AGGV_NDIMS; i++)
        if (d[i] < 0 || d[i] > (1 << 20)) return false;
    s.N = (size_t)d[0]; s.k = (size_t)d[1]; s.nd = (size_t)d[2]; s.np = (size_t)d[3]; s.rounds = (size_t)d[4]; s.nl = (size_t)d[5];
    s.nn = (size_t)d[6]; s.NG = (size_t)d[7]; s.NH = (size_t)d[8]; s.form = (uint32_t)d[9]; s.W = (size_t)d[10]; s.label_len = (size_t)d[11];
    s.G = (int)(s.form & 0xFu); s.fb = (int)((s.form >> 4) & 0xFu); s.tables = (s.form & AGGV_FORM_TABLES) != 0;
    s.proof_bytes = 64 * (4 + 2 * s.rounds + s.k) + 32 * (s.nl + s.nn);
    if (s.N < 1 || s.N > AGG_MAX_N || s.k < 1 || s.k > 64 || s.nd < 1 || s.np < 1 || s.np > s.nd + 1 || s.k * s.nd > s.NG || s.nd + 10 > s.NH ||
        s.rounds > 12 || s.nl > 4096 || s.nn > 4096 || s.W != 4 || s.label_len < 1 || s.label_len > 255)
        return false;
    if (4 + s.k > 8 * 5) return false;      // fallback_mask has a bit for each of 8 chunks of five points
    if ((s.form >> 9) != 0 || !(s.G == 1 || s.G == 2 || s.G == 4 || s.G == 8) || s.fb > AGGV_FB_L64) return false;
    return true;
}
inline void verify_sizes(const VerifyShape& s, size_t in_bytes[4], size_t io_bytes[AGGV_NBUFS]) {
    const size_t N = s.N, nm = s.k * s.nd;
    in_bytes[0] = s.label_len; in_bytes[1] = (1 + s.NG + s.NH) * bppp::fb_per_base((int)s.W) * sizeof(bppp::apt_packed);
    in_bytes[2] = N * s.k * 64; in_bytes[3] = N * s.proof_bytes;
    io_bytes[V_STATUS] = N * 4; io_bytes[V_TSTATE] = 52 * N * 4; io_bytes[V_SC0] = (nm + 5 + s.k) * 8 * N * 4;
    io_bytes[V_PTS] = (4 + s.k) * 16 * N * 4; io_bytes[V_ACC] = 30 * N * 4; io_bytes[V_PFIX] = 30 * N * 4; io_bytes[V_INV] = s.np * 8 * N * 4;
    io_bytes[V_VSUM] = s.k * 40 * N * 4; io_bytes[V_COMMIT] = N * 64; io_bytes[V_C] = N * s.NH * 32; io_bytes[V_RHO] = N * 32;
    io_bytes[V_MU] = N * 32; io_bytes[V_FELL] = N;
}
// scratch the stages keep to themselves: window tables of the 4 + k points (entry-major), the running products of their build, and the
// projective tables of the other form
inline size_t verify_atab_entries(const VerifyShape& s) { return (4 + s.k) * 16 * s.N; }
inline size_t verify_tscr_words(const VerifyShape& s) { return (size_t)BPPP_TSCR_PER_POINT * (4 + s.k) * 10 * s.N; }
inline size_t verify_straus_slots(const VerifyShape& s) { return s.N * 5 * BPPP_STRAUS_ENTRIES; }

// the workspace as agg_ws_fill of bppp_generic.hip fills it, over the caller's buffers; the tables of the 4 + k points
// start at entry 0 (no round points in front of them)
inline bppp::AggWs verify_ws(const VerifyShape& s, const uint8_t* label, const void* table, const void* com, const void* proofs, void* const* io,
                             bppp::apt_packed* atab, bppp::u32* tscr, bppp::pt_slot* straus) {
    using bppp::u32;
    bppp::AggWs r;
    memset(&r, 0, sizeof r);
    r.N = s.N; r.k = (int)s.k; r.nd = (int)s.nd; r.np = (int)s.np; r.rounds = (int)s.rounds; r.nl = (int)s.nl; r.nn = (int)s.nn;
    r.NG = (int)s.NG; r.NH = (int)s.NH; r.proof_bytes = s.proof_bytes;
    r.commitments = (const uint8_t*)com; r.proofs = (const uint8_t*)proofs;
    r.status = (int32_t*)io[V_STATUS]; r.tstate = (u32*)io[V_TSTATE]; r.sc0 = (u32*)io[V_SC0]; r.pts = (u32*)io[V_PTS]; r.acc = (u32*)io[V_ACC];
    r.pfix = (u32*)io[V_PFIX]; r.inv = (u32*)io[V_INV]; r.vsum = (u32*)io[V_VSUM];
    r.wn_commit = (uint8_t*)io[V_COMMIT]; r.wn_c = (uint8_t*)io[V_C]; r.wn_rho = (uint8_t*)io[V_RHO]; r.wn_mu = (uint8_t*)io[V_MU];
    r.straus = straus;
    r.atab = s.tables ? atab : nullptr; r.tscr = tscr; r.atab_first = 0;
    r.fb.table = (const bppp::apt_packed*)table; r.fb.W = (int)s.W; r.fb.N = s.N;
    bppp::t_new(r.base, label, (u32)s.label_len);
    return r;
}

// agg_c0_chunk with straus_affine_fast in place of straus_affine: true when the chunk's fast sum met an exceptional addition
template <int M>
HD bool chunk_falls_back(const bppp::AggWs& w, size_t t, int first) {
    int pslot[M];
    bppp::glv_words<M> g;
#pragma unroll
    for (int j = 0; j < M; j++) {
        pslot[j] = first + j;
        bppp::sc kk;
        bppp::ws_ld8(kk.v, w.sc0, w.N, t, 1 + w.k * w.nd + first + j);
        bppp::glv_split sp;
        bppp::glv_decompose(sp, kk);
        bppp::glv_words_set<M>(g, j, sp);
    }
    bppp::pt scratch;
    return !bppp::straus_affine_fast<M>(scratch, bppp::atab_of(w.atab, w.N, t) + w.atab_first, pslot, g);
}
// bit c: chunk c of agg_c0_var's walk over the window tables took the complete-formula fallback
HD uint8_t fallback_mask(const bppp::AggWs& w, size_t t) {
    const int npts = 4 + w.k;
    uint8_t mask = 0;
    if (!w.atab) return 0;
    for (int first = 0, c = 0; first < npts && c < 8; first += 5, c++) {
        const int m = npts - first < 5 ? npts - first : 5;
        bool fb;
        switch (m) {
        case 5: fb = chunk_falls_back<5>(w, t, first); break;
        case 4: fb = chunk_falls_back<4>(w, t, first); break;
        case 3: fb = chunk_falls_back<3>(w, t, first); break;
        case 2: fb = chunk_falls_back<2>(w, t, first); break;
        default: fb = chunk_falls_back<1>(w, t, first); break;
        }
        if (fb) mask |= (uint8_t)(1u << c);
    }
    return mask;
}

struct ProveShape {
    size_t N, k, nd, np, NG, NH, label_len, n_rnd;
    int stages;
};
inline bool prove_shape(ProveShape& s, const int64_t* d) {
    for (int i = 0; i < AGGP_NDIMS; i++)
        if (d[i] < 0 || d[i] > (1 << 20)) return false;
    s.N = (size_t)d[0]; s.k = (size_t)d[1]; s.nd = (size_t)d[2]; s.np = (size_t)d[3]; s.NG = (size_t)d[4]; s.NH = (size_t)d[5];
    s.stages = (int)d[6]; s.label_len = (size_t)d[7];
    if (s.N < 1 || s.N > AGG_MAX_N || s.label_len < 1 || s.label_len > 255 || (s.stages & ~(AGGP_WITNESS | AGGP_R1 | AGGP_MSM | AGGP_R2 | AGGP_CT)) ||
        !(s.stages & ~AGGP_CT))
        return false;
    // the witness stage alone reads no generator and takes any base the digit routine takes (np > nd + 1 included); the other stages need
    // the shape the entry points accept
    if ((s.stages & ~AGGP_CT) == AGGP_WITNESS) {
        if (s.k < 1 || s.k > 64 || s.nd < 1 || s.nd > 256 || s.np < 1 || !bppp::recip_values_shape_ok(s.nd, s.np)) return false;
    } else if (!bppp::agg_prove_shape_ok(s.k, s.nd, s.np, s.NG, s.NH)) {
        return false;
    }
    s.n_rnd = bppp::agg_prove_draws(s.k, s.nd);
    return true;
}
inline void prove_sizes(const ProveShape& s, size_t io_bytes[AGGP_NBUFS]) {
    const size_t N = s.N, rows = N * s.k, nm = s.k * s.nd, nv = s.nd + 1;
    io_bytes[P_X] = rows * 32; io_bytes[P_S] = rows * 32; io_bytes[P_RND] = N * s.n_rnd * 32; io_bytes[P_COM] = rows * 64;
    io_bytes[P_DIGITS] = N * nm * 32; io_bytes[P_M] = N * s.np * 32; io_bytes[P_STATUS] = N * 4; io_bytes[P_ROW_STATUS] = rows * 4;
    io_bytes[P_VSC] = 2 * 8 * rows * 4; io_bytes[P_TSTATE] = 52 * N * 4; io_bytes[P_INST] = (2 + s.np) * 8 * N * 4;
    io_bytes[P_SCR] = (nm + s.np) * 8 * N * 4; io_bytes[P_RSC] = nv * 8 * rows * 4; io_bytes[P_RPB] = 30 * rows * 4;
    io_bytes[P_VSUM] = s.k * 50 * N * 4; io_bytes[P_CP_V] = rows * nv * 32; io_bytes[P_CP_SV] = rows * 32; io_bytes[P_CP_WR] = N * nm * 32;
    io_bytes[P_CP_VPTS] = rows * 64; io_bytes[P_PROOF_R] = rows * 64;
}
inline size_t prove_table_bytes(const ProveShape& s) { return (1 + s.NG + s.NH) * bppp::fb_per_base(4) * sizeof(bppp::apt_packed); }
// the workspace as agg_prove_part of bppp_generic.hip fills it as far as the four stages read it
inline bppp::AggProveWs prove_ws(const ProveShape& s, const uint8_t* label, const void* table, void* const* io) {
    using bppp::u32;
    bppp::AggProveWs a;
    memset(&a, 0, sizeof a);
    a.N = s.N; a.k = (int)s.k; a.nd = (int)s.nd; a.np = (int)s.np; a.NG = (int)s.NG; a.NH = (int)s.NH; a.n_rnd = (int)s.n_rnd;
    bppp::recip_witness_shape(a.rw, s.nd, s.np);
    a.x = (const uint8_t*)io[P_X]; a.s = (const uint8_t*)io[P_S]; a.rnd = (const uint8_t*)io[P_RND]; a.commitments = (const uint8_t*)io[P_COM];
    a.digits = (uint8_t*)io[P_DIGITS]; a.m = (uint8_t*)io[P_M]; a.status = (int32_t*)io[P_STATUS]; a.row_status = (int32_t*)io[P_ROW_STATUS];
    a.vsc = (u32*)io[P_VSC]; a.tstate = (u32*)io[P_TSTATE]; a.inst_vals = (u32*)io[P_INST]; a.scr = (u32*)io[P_SCR]; a.rsc = (u32*)io[P_RSC];
    a.rpb = (u32*)io[P_RPB]; a.vsum = (u32*)io[P_VSUM]; a.cp_v = (uint8_t*)io[P_CP_V]; a.cp_sv = (uint8_t*)io[P_CP_SV];
    a.cp_wr = (uint8_t*)io[P_CP_WR]; a.cp_vpts = (uint8_t*)io[P_CP_VPTS]; a.proof_R = (uint8_t*)io[P_PROOF_R];
    a.fb.table = (const bppp::apt_packed*)table; a.fb.W = 4; a.fb.N = s.N * s.k;
    a.fb_ct = a.fb;
    a.ct = (s.stages & AGGP_CT) ? 1 : 0;
    bppp::t_new(a.base, label, (u32)s.label_len);
    return a;
}

}  // namespace aggp
