// TEST-ONLY host build of the primitive dispatcher (prims_core.h), one record after another.  Built twice by tests/prims/build.py:
// g++ (libbppp_prims_gcc.so: the code path of the tests/emul emulation) and ROCm's clang++ (libbppp_prims_clang.so: the
// __builtin_addc / __builtin_subc carry chains of the device build).  Both carry the magnitude in every field element and assert it.
#include <assert.h>
#include <execinfo.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "prims_core.h"
#include "bucket_prims.h"
#include "agg_prims.h"
#include "circuit_prims.h"

#define PRIMS_API extern "C" __attribute__((visibility("default")))

PRIMS_API int prims_record_words(int which) { return which == 0 ? PRIM_IN_WORDS : PRIM_OUT_WORDS; }
// 1 when this library was compiled by clang (the addc/subc builtins path of field.h), 0 for g++
PRIMS_API int prims_is_clang(void) {
#if defined(__clang__)
    return 1;
#else
    return 0;
#endif
}
PRIMS_API int prims_run_host(const uint32_t* in, uint32_t* out, size_t n, const uint8_t* bytes, size_t nbytes) {
    for (size_t r = 0; r < n; r++) {
        const uint32_t* rin = in + r * PRIM_IN_WORDS;
        prims::prim_eval(rin[0], rin, out + r * PRIM_OUT_WORDS, bytes, nbytes);
    }
    return 0;
}

// The one-lane forms of the variable-base sums (prims_core.h: SumForm), one record after another with a workspace of its own (N = 1).
template <int M>
static void sums_host(uint32_t cfg, const uint32_t* in, uint32_t* out, size_t n) {
    const uint32_t form = cfg & 0xFFu, parts = cfg >> 24, np = parts ? parts : 1;
    std::vector<uint32_t> pts(16 * M), tscr(BPPP_TSCR_PER_POINT * M * 10);
    std::vector<bppp::apt_packed> atab((size_t)np * M * 16);
    const prims::SumWs w = {1, pts.data(), tscr.data(), atab.data()};
    for (size_t r = 0; r < n; r++) {
        const uint32_t* rec = in + r * SUM_IN_WORDS;
        uint32_t* o = out + r * SUM_OUT_WORDS;
        if (rec[0] != cfg) { o[SUM_OUT_WORDS - 1] = prims::ST_BAD_PARAM; continue; }
        if (form == prims::SUM_SPLIT_LANES) {
            for (int slot = 0; slot < (int)parts * M; slot++) prims::sum_table_one<M>(w, 0, rec, slot, (int)parts);
        } else {
            prims::sum_tables_build<M>(w, 0, rec);
        }
        prims::sum_one_lane<M>(form, (int)parts, w, 0, rec, o);
        o[SUM_OUT_WORDS - 1] = prims::ST_OK;
    }
}
PRIMS_API int prims_sum_words(int which) { return which == 0 ? SUM_IN_WORDS : SUM_OUT_WORDS; }
// n records of one configuration (cfg = prims::sum_cfg).  Returns 0, or -1 for a configuration the host cannot run.
PRIMS_API int prims_run_sums_host(uint32_t cfg, const uint32_t* in, uint32_t* out, size_t n) {
    if (!prims::sum_cfg_ok(cfg) || (cfg & 0xFFu) >= prims::SUM_GROUP) return -1;
    switch ((cfg >> 8) & 0xFFu) {
    case 1: sums_host<1>(cfg, in, out, n); break;
    case 2: sums_host<2>(cfg, in, out, n); break;
    case 3: sums_host<3>(cfg, in, out, n); break;
    case 4: sums_host<4>(cfg, in, out, n); break;
    default: sums_host<5>(cfg, in, out, n); break;
    }
    return 0;
}

// The transcript primitives (prims_core.h: TrStep), one record after another on the register sponge -- the only form the host has; the
// launch layouts are a device matter.  Returns 0, or -1 for a form the host cannot run.
PRIMS_API int prims_transcript_words(int which) { return which == 0 ? TR_IN_WORDS : which == 1 ? TR_OUT_WORDS : TR_PROG_WORDS; }
PRIMS_API int prims_run_transcript_host(const uint32_t* prog, uint32_t form, uint32_t layout, const uint8_t* states, const uint32_t* in,
                                        uint32_t* out, size_t n) {
    if (form != prims::TR_REGS || layout > prims::TR_GROUPED) return -1;
    const bool ok = prims::tr_prog_ok(prog, form);
    for (size_t r = 0; r < n; r++) {
        uint32_t* o = out + r * TR_OUT_WORDS;
        if (!ok) { o[51] = prims::ST_BAD_PARAM; continue; }
        prims::tr_eval_regs(prog, states + r * BPPP_TRANSCRIPT_STATE_BYTES, in + r * TR_IN_WORDS, o);
    }
    return 0;
}

// The bucket stage of the RLC batch mode (bucket_prims.h has the arguments) in the single-thread form of bucket_core.h: bkt_prepare per
// proof, then bkt_superchunk_serial per superchunk (plain bucket sums, bkt_mac / bkt_finish_scalar, fb_sum_serial), and k_bkt_check's
// verdict bytes.  Returns 0, or -1 for arguments out of range.
PRIMS_API size_t prims_bucket_fb_entries(int nb, int W) { return bktp::fb_entries(nb, W); }
PRIMS_API int prims_bucket_fb_build(const uint8_t* gens, int nb, int W, uint8_t* table_out) {
    if (nb < 1 || nb > BKT_MAX_NB || W != 4) return -1;
    return bktp::fb_build(gens, nb, W, table_out);
}
// {dynamic LDS bytes of k_bkt_accumulate, base groups of k_bkt_scalars}: the launch geometry the product and the launcher share
PRIMS_API void prims_bucket_geometry(uint32_t M, int nb, uint64_t out[2]) { out[0] = bppp::bkt_lds_bytes(M); out[1] = bppp::bkt_scalar_groups(nb); }
PRIMS_API int prims_run_bucket_host(size_t N, uint32_t M, int nb, const uint64_t* seed, const int32_t* status, const uint32_t* acc,
                                    const uint32_t* fsc, const uint8_t* table, int W, int given, uint64_t* wab, uint32_t* c4, uint32_t* lhs,
                                    uint32_t* asc, uint8_t* sflag, uint8_t* accept) {
    if (!bktp::args_ok(N, M, nb, W)) return -1;
    const size_t ns = bktp::nsuper_of(N, M);
    for (size_t c = 0; c < ns; c++) sflag[c] = BKT_SENTINEL;
    for (size_t j = 0; j < N; j++) accept[j] = BKT_SENTINEL;
    const bppp::BucketWs w = bktp::workspace(N, M, nb, seed, status, acc, fsc, table, W, wab, c4, lhs, asc, sflag, accept);
    if (!given)
        for (size_t t = 0; t < N; t++) bppp::bkt_prepare(w, t);
    for (size_t c = 0; c < ns; c++) {
        const bool ok = bppp::bkt_superchunk_serial(w, c);
        sflag[c] = ok ? 0 : 1;
        if (ok)
            for (size_t j = c * M; j < c * M + M && j < N; j++) accept[j] = status[j] == bppp::ST_OK ? 1 : 0;
    }
    return 0;
}

// The aggregate verifier's phase 1 and C0 stage (agg_prims.h has the arguments) in the single-thread form of agg_core.h, as
// tests/emul/agg_emul.cpp walks it: the G runs of an instance one after the other (last first) with their sums added here, where the
// device adds them by shuffles; the fixed-base half as fb_sum_serial over the form's lane count (1, BPPP_FB_LANES, 64); the
// variable-base half on the window tables or on the projective tables.  Returns 0, or -1 for arguments out of range.
PRIMS_API int prims_run_agg_verify_host(const int64_t* dims, const void* const* in, void* const* io) {
    using namespace bppp;
    aggp::VerifyShape s;
    if (!aggp::verify_shape(s, dims)) return -1;
    std::vector<apt_packed> atab(aggp::verify_atab_entries(s));
    std::vector<u32> tscr(aggp::verify_tscr_words(s));
    std::vector<pt_slot> straus(aggp::verify_straus_slots(s));
    const AggWs r = aggp::verify_ws(s, (const uint8_t*)in[0], in[1], in[2], in[3], io, atab.data(), tscr.data(), straus.data());
    const size_t n = s.N;
    for (size_t t = 0; t < n; t++) {
        if (s.G == 1) { agg_phase1(r, t); continue; }
        AggHead h;
        sc ps, musum, p, m;
        agg_phase1_head(r, t, h);
        sc_set_u32(ps, 0); sc_set_u32(musum, 0);
        for (int q = s.G - 1; q >= 0; q--) { agg_phase1_run(r, t, h, q, s.G, p, m); sc_add(ps, ps, p); sc_add(musum, musum, m); }
        agg_phase1_tail(r, t, h, ps, musum);
    }
    const int lanes = s.fb == AGGV_FB_L1 ? 1 : s.fb == AGGV_FB_L64 ? 64 : BPPP_FB_LANES;
    for (size_t t = 0; t < n; t++) {
        pt a;
        FbRanges rg;
        agg_c0_fixed_ranges(rg, r);
        fb_sum_serial(a, r.fb, t, r.sc0, rg, lanes);
        agg_c0_fixed_store(r, t, a);
    }
    if (r.atab) for (size_t t = 0; t < n; t++) agg_c0_tables(r, t);
    for (size_t t = 0; t < n; t++) agg_c0_var(r, t);
    for (size_t t = 0; t < n; t++) ((uint8_t*)io[aggp::V_FELL])[t] = aggp::fallback_mask(r, t);
    for (size_t t = 0; t < n; t++) agg_c0_finish(r, t);
    return 0;
}

// The aggregate prover's witness, r1, msm and r2 stages, each over all instances (the msm: all N k rows, a serial fixed-base sum per
// row) before the next.  Returns 0, or -1 for arguments out of range.
PRIMS_API int prims_run_agg_prove_host(const int64_t* dims, const void* const* in, void* const* io) {
    aggp::ProveShape s;
    if (!aggp::prove_shape(s, dims)) return -1;
    if ((s.stages & AGGP_MSM) && !in[1]) return -1;
    const bppp::AggProveWs a = aggp::prove_ws(s, (const uint8_t*)in[0], in[1], io);
    if (s.stages & AGGP_WITNESS) for (size_t t = 0; t < s.N; t++) bppp::agg_prove_witness(a, t);
    if (s.stages & AGGP_R1) for (size_t t = 0; t < s.N; t++) bppp::agg_prove_stage_r1(a, t);
    if (s.stages & AGGP_MSM) {
        const size_t rows = s.N * s.k;
        bppp::FbRanges rg;
        bppp::agg_prove_pole_ranges(rg, a);
        for (size_t row = 0; row < rows; row++) {
            bppp::pt acc;
            if (a.ct) bppp::fb_sum_serial_ct(acc, a.fb_ct, row, a.rsc, rg);
            else bppp::fb_sum_serial(acc, a.fb, row, a.rsc, rg);
            bppp::ws_st_pt(a.rpb, rows, row, acc);
        }
    }
    if (s.stages & AGGP_R2) for (size_t t = 0; t < s.N; t++) bppp::agg_prove_stage_r2(a, t);
    return 0;
}

// The circuit verifier's phase 1 and C0 stage (circuit_prims.h has the arguments) in the single-thread form of circuit_core.h, as
// tests/emul/bppp_emul.cpp walks it: the fixed-base half as fb_sum_serial over the plan's lane count (64 or BPPP_FB_LANES), the
// variable-base half on the window tables or on the projective tables.  The lane-per-point form meets by shuffles and has no host
// form.  Returns 0, or -1 for arguments out of range.
PRIMS_API int prims_run_circuit_host(const int64_t* dims, const void* const* in, void* const* io) {
    using namespace bppp;
    circp::Shape s;
    if (!circp::shape(s, dims) || s.form == CIRC_VAR_POINTS) return -1;
    CircuitHostData hd;
    if (!circp::host_data(hd, s, in)) return -1;
    const void* arr[9];
    size_t arr_bytes[9];
    circp::host_arrays(hd, arr, arr_bytes);
    std::vector<apt_packed> atab(circp::atab_entries(s));
    std::vector<u32> tscr(circp::tscr_words(s));
    std::vector<pt_slot> straus(circp::straus_slots(s));
    const CircuitWs r = circp::workspace(s, (const uint8_t*)in[circp::I_LABEL], in[circp::I_TABLE], in[circp::I_COM], in[circp::I_PROOFS], arr, io,
                                         atab.data(), tscr.data(), straus.data());
    const size_t n = s.N;
    for (size_t t = 0; t < n; t++) circuit_phase1(r, t);
    const int lanes = s.plan.fb == bppp_host::GENERIC_FB_WAVEFRONT ? 64 : BPPP_FB_LANES;
    for (size_t t = 0; t < n; t++) {
        pt a;
        FbRanges rg;
        circuit_c0_fixed_ranges(rg, r);
        fb_sum_serial(a, r.fb, t, r.sc0, rg, lanes);
        circuit_c0_fixed_store(r, t, a);
    }
    if (r.atab) for (size_t t = 0; t < n; t++) circuit_c0_tables(r, t);
    for (size_t t = 0; t < n; t++) circuit_c0_var(r, t);
    for (size_t t = 0; t < n; t++) circuit_c0_finish(r, t);
    circp::plan_words(s, (int32_t*)io[circp::B_PLAN]);
    return 0;
}
// plan_generic's choices for a circuit verify call of n instances on the default knobs (circuit_prims.h: plan_words), or with
// no_lane_groups / slow_rounds set as BPPP_NO_LANE_GROUPS / BPPP_GENERIC_SLOW_ROUNDS set them: what "last_generic_form" of a call through
// the C ABI is compared with
PRIMS_API void prims_circuit_plan(size_t n, size_t rounds, size_t k, int no_lane_groups, int slow_rounds, int32_t out[CIRC_PLAN_WORDS]) {
    bppp_host::GenericKnobs knobs;
    knobs.no_lane_groups = no_lane_groups != 0;
    knobs.slow_rounds = slow_rounds != 0;
    circp::Shape s{};
    s.plan = bppp_host::plan_generic(bppp_host::GENERIC_FORM_CIRCUIT, n, rounds, knobs, n, 1, 4 + k);
    circp::plan_words(s, out);
}
