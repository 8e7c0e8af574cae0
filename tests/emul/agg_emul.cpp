// TEST-ONLY host emulation of the aggregated reciprocal range proof verifier's device code (bp_pp_amd/csrc/agg_core.h, then the
// generic WNLA stage of wnla_core.h): the exact __host__ __device__ functions the kernels of k_agg.hip call, compiled with g++ and run
// one "thread" after the other.  A translation unit of its own beside bppp_emul.cpp (tests/emul/build_agg.py builds it); the
// fixed-base table it takes is the one bppp_emul.cpp's emul_fb_build makes.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../bp_pp_amd/csrc/plan_core.h"      // (before the device headers: field.h pulls <stdio.h> in inside its namespace in the host build)
#include "../../bp_pp_amd/csrc/agg_core.h"

using namespace bppp;

extern "C" {

// The plan of a generic verify call as the library takes it (plan_core.h: plan_generic), for the CPU test of its thresholds:
// out = code, p1_group, fb, beside, c0var_group, c0_chunks, round_group, tab_parts, final_lg, per_point
void emul_agg_plan(int protocol, size_t n, size_t rounds, int n_simds, int timing, int lane_group, size_t c0_points, unsigned out[10]) {
    bppp_host::GenericKnobs k;
    k.n_simds = n_simds; k.timing = timing != 0; k.lane_group = lane_group;
    const bppp_host::GenericPlan p = bppp_host::plan_generic(protocol, n, rounds, k, n, 1, c0_points);
    out[0] = p.code(); out[1] = (unsigned)p.p1_group; out[2] = (unsigned)p.fb; out[3] = p.beside ? 1u : 0u; out[4] = (unsigned)p.c0var_group;
    out[5] = (unsigned)p.c0_chunks; out[6] = (unsigned)p.round_group; out[7] = (unsigned)p.tab_parts; out[8] = (unsigned)p.final_lg;
    out[9] = p.per_point ? 1u : 0u;
}

// Aggregated reciprocal verify, every stage in thread order.  G: lanes per instance of phase 1 (1, 2, 4, 8): the G runs of an instance
// are walked one after the other (last first) and their sums added here, where the device adds them by shuffles.  slow != 0: the
// projective-table forms of C0's variable-base sum and of the rounds.  Out, for the comparison with the oracle's trace:
// rho, mu [n x 32], c [n x NH x 32], ps_tau | pn_tau [n x (1 + k nd) x 32] (big-endian), C0 [n x 64], phase 1's status [n].
int emul_agg_verify(const uint8_t* table, int W, int NG, int NH, int k, int nd, int np, const uint8_t* label, size_t label_len, size_t n,
                    const uint8_t* commitments, const uint8_t* proofs, int rounds, int nl, int nn, int G, int slow, uint8_t* out_rho,
                    uint8_t* out_mu, uint8_t* out_c, uint8_t* out_pn, uint8_t* out_c0, int32_t* out_p1_status, uint8_t* accept,
                    int32_t* status) {
    const size_t T = (size_t)1 << rounds, NB = 1 + (size_t)NG + NH, nm = (size_t)k * nd;
    const size_t proof_bytes = 64 * (4 + 2 * (size_t)rounds + k) + 32 * ((size_t)nl + nn);
    AggWs r;
    memset(&r, 0, sizeof r);
    r.N = n; r.k = k; r.nd = nd; r.np = np; r.rounds = rounds; r.nl = nl; r.nn = nn; r.NG = NG; r.NH = NH; r.proof_bytes = proof_bytes;
    r.commitments = commitments; r.proofs = proofs; r.status = status;
    std::vector<u32> ts(52 * n), sc0((nm + 5 + k) * 8 * n), pts((size_t)(4 + k) * 16 * n), acc(30 * n), pf(30 * n), inv((size_t)np * 8 * n),
        vs((size_t)k * 40 * n), ys((rounds ? rounds : 1) * 8 * n), tab(2 * T * 8 * n), msc(NB * 8 * n);
    std::vector<pt_slot> straus(n * 5 * BPPP_STRAUS_ENTRIES);
    r.tstate = ts.data(); r.sc0 = sc0.data(); r.pts = pts.data(); r.acc = acc.data(); r.pfix = pf.data(); r.inv = inv.data();
    r.vsum = vs.data(); r.straus = straus.data();
    r.wn_commit = out_c0; r.wn_c = out_c; r.wn_rho = out_rho; r.wn_mu = out_mu;
    r.fb.table = (const apt_packed*)table; r.fb.W = W; r.fb.N = n;
    t_new(r.base, label, (u32)label_len);
    WnlaWs w;
    memset(&w, 0, sizeof w);
    w.N = n; w.ng = NG; w.nh = NH; w.rounds = rounds; w.nl = nl; w.nn = nn;
    w.base = r.base; w.tio = r.tio;
    w.commitments = r.wn_commit; w.c = r.wn_c; w.rho = r.wn_rho; w.mu = r.wn_mu;
    w.proof_r = proofs + 256; w.proof_x = proofs + 256 + 64 * (size_t)rounds; w.proof_l = proofs + 64 * (size_t)(4 + k) + 128 * (size_t)rounds;
    w.proof_n = w.proof_l + 32 * (size_t)nl;
    w.stride_r = w.stride_x = w.stride_l = w.stride_n = proof_bytes;
    w.transcript_preloaded = 1;
    w.accept = accept; w.status = status; w.tstate = r.tstate; w.acc = r.acc; w.pfix = r.pfix; w.ys = ys.data(); w.tab = tab.data();
    w.msc = msc.data(); w.straus = straus.data(); w.fb = r.fb;
    for (size_t t = 0; t < n; t++) {
        if (G <= 1) { agg_phase1(r, t); continue; }
        AggHead h;
        sc ps, musum, p, m;
        agg_phase1_head(r, t, h);
        sc_set_u32(ps, 0); sc_set_u32(musum, 0);
        for (int q = G - 1; q >= 0; q--) { agg_phase1_run(r, t, h, q, G, p, m); sc_add(ps, ps, p); sc_add(musum, musum, m); }
        agg_phase1_tail(r, t, h, ps, musum);
    }
    for (size_t t = 0; t < n; t++) {
        out_p1_status[t] = status[t];
        for (size_t j = 0; j <= nm; j++) { sc v; ws_ld8(v.v, r.sc0, n, t, (int)j); sc_to_be(out_pn + (t * (nm + 1) + j) * 32, v); }
    }
    for (size_t t = 0; t < n; t++) {
        pt a;
        FbRanges rg;
        agg_c0_fixed_ranges(rg, r);
        fb_sum_serial(a, r.fb, t, r.sc0, rg);
        agg_c0_fixed_store(r, t, a);
    }
    // as agg_verify_device_impl: the 4 + k points' tables behind the round points'
    std::vector<apt_packed> atab;
    std::vector<u32> tscr, rpts;
    if (rounds != 0 && !slow) {
        const size_t npts = 2 * (size_t)rounds + 4 + k;
        atab.assign(npts * 16 * n, apt_packed());
        tscr.assign((size_t)BPPP_TSCR_PER_POINT * npts * 10 * n, 0u);
        rpts.assign(npts * 16 * n, 0u);
        w.atab = atab.data(); w.tscr = tscr.data(); w.rpts = rpts.data();
    }
    r.atab = w.atab; r.tscr = w.tscr; r.atab_first = 2 * rounds * 16;
    if (r.atab) for (size_t t = 0; t < n; t++) agg_c0_tables(r, t);
    for (size_t t = 0; t < n; t++) agg_c0_var(r, t);
    for (size_t t = 0; t < n; t++) agg_c0_finish(r, t);
    std::vector<uint8_t> c0(out_c0, out_c0 + 64 * n);      // (the WNLA stage reads the commitment in place)
    for (size_t t = 0; t < n; t++) wnla_verify_begin(w, t);
    if (w.atab) for (size_t t = 0; t < n; t++) wnla_verify_tables(w, t);
    for (int kk = 1; kk <= rounds; kk++)
        for (size_t t = 0; t < n; t++) wnla_verify_round(w, t, kk);
    for (size_t t = 0; t < n; t++) wnla_verify_final_scalars(w, t);
    for (size_t t = 0; t < n; t++) {
        pt a;
        FbRanges rg;
        wnla_msm_ranges(rg, w);
        fb_sum_serial(a, w.fb, t, w.msc, rg);
        wnla_verify_store(w, t, a);
    }
    for (size_t t = 0; t < n; t++) wnla_verify_accept(w, t);
    memcpy(out_c0, c0.data(), 64 * n);
    return 0;
}

}  // extern "C"
