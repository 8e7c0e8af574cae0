// TEST-ONLY host emulation of the mixed-value-count aggregate verifier's device code (bp_pp_amd/csrc/agg_mixed_core.h, then the uniform
// fixed-base half, finish and WNLA stage): the exact __host__ __device__ functions the kernels of k_agg_mixed.hip call, compiled with
// g++ and run one "thread" after the other in the order of agg_verify_device_impl's mixed form.  A translation unit of its own beside agg_emul.cpp
// (tests/emul/build_agg_mixed.py builds it); the fixed-base table it takes is the one bppp_emul.cpp's emul_fb_build makes.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../bp_pp_amd/csrc/plan_core.h"      // (before the device headers: field.h pulls <stdio.h> in inside its namespace in the host build)
#include "../../bp_pp_amd/csrc/agg_mixed_core.h"

using namespace bppp;

static void phase1_all(const AggMixedWs& m, size_t n, int G) {
    for (size_t t = 0; t < n; t++) {
        if (G <= 1) { agg_mixed_phase1(m, t); continue; }
        AggHead h;
        sc ps, musum, p, s;
        bool bad;
        const int k = agg_mixed_k(m, t, bad);
        agg_mixed_phase1_head(m, t, k, bad, h);
        sc_set_u32(ps, 0); sc_set_u32(musum, 0);
        for (int q = G - 1; q >= 0; q--) { agg_mixed_phase1_run(m, t, k, h, q, G, p, s); sc_add(ps, ps, p); sc_add(musum, musum, s); }
        agg_mixed_phase1_tail(m, t, k, h, ps, musum);
    }
}

extern "C" {

// Mixed aggregate verify, every stage in thread order.  ks [n]; commitments n x k_max x 64 and proofs n x proof_bytes(k_max) slots.
// G: lanes per instance of phase 1 (the G runs walked last first, their sums added here).  slow != 0: the projective-table forms.
// nl_fixed: the lanes of the fixed-base half (1, 8, 64).  prev_ks (or null): phase 1 is run with THESE counts first, on the same
// workspace and inputs -- the call before this one, whose entries the second run has to overwrite.
// Out: rho, mu [n x 32], c [n x NH x 32], C0 [n x 64], phase 1's status [n], accept, status, and the workspace as phase 1 left it,
// word for word: sc0 [(k_max nd + 5 + k_max) * 8][n], pts [(4 + k_max) * 16][n], ln [n][32 (nl + nn)], e^-1 [8][n].
int emul_agg_mixed_verify(const uint8_t* table, int W, int NG, int NH, int k_max, int nd, int np, const uint8_t* label, size_t label_len,
                          size_t n, const uint8_t* ks, const uint8_t* prev_ks, const uint8_t* commitments, const uint8_t* proofs, int rounds,
                          int nl, int nn, int G, int slow, int nl_fixed, uint8_t* out_rho, uint8_t* out_mu, uint8_t* out_c, uint8_t* out_c0,
                          int32_t* out_p1_status, uint8_t* accept, int32_t* status, u32* out_sc0, u32* out_pts, uint8_t* out_ln,
                          u32* out_einv) {
    const size_t T = (size_t)1 << rounds, NB = 1 + (size_t)NG + NH, nm = (size_t)k_max * nd, k = (size_t)k_max;
    const size_t proof_bytes = 64 * (4 + 2 * (size_t)rounds + k) + 32 * ((size_t)nl + nn);
    AggMixedWs m;
    memset(&m, 0, sizeof m);
    AggWs& r = m.w;
    r.N = n; r.k = k_max; r.nd = nd; r.np = np; r.rounds = rounds; r.nl = nl; r.nn = nn; r.NG = NG; r.NH = NH; r.proof_bytes = proof_bytes;
    r.commitments = commitments; r.proofs = proofs; r.status = status;
    std::vector<u32> ts(52 * n), sc0((nm + 5 + k) * 8 * n), pts((size_t)(4 + k) * 16 * n), acc(30 * n), pf(30 * n), inv((size_t)np * 8 * n),
        vs((size_t)k * 40 * n), ys((rounds ? rounds : 1) * 8 * n), tab(2 * T * 8 * n), msc(NB * 8 * n);
    std::vector<uint8_t> ln((size_t)32 * (nl + nn) * n);
    std::vector<pt_slot> straus(n * 5 * BPPP_STRAUS_ENTRIES);
    r.tstate = ts.data(); r.sc0 = sc0.data(); r.pts = pts.data(); r.acc = acc.data(); r.pfix = pf.data(); r.inv = inv.data();
    r.vsum = vs.data(); r.straus = straus.data();
    r.wn_commit = out_c0; r.wn_c = out_c; r.wn_rho = out_rho; r.wn_mu = out_mu;
    r.fb.table = (const apt_packed*)table; r.fb.W = W; r.fb.N = n;
    t_new(r.base, label, (u32)label_len);
    m.ln = ln.data();
    WnlaWs w;
    memset(&w, 0, sizeof w);
    w.N = n; w.ng = NG; w.nh = NH; w.rounds = rounds; w.nl = nl; w.nn = nn;
    w.base = r.base; w.tio = r.tio;
    w.commitments = r.wn_commit; w.c = r.wn_c; w.rho = r.wn_rho; w.mu = r.wn_mu;
    w.proof_r = proofs + 256; w.proof_x = proofs + 256 + 64 * (size_t)rounds;
    w.stride_r = w.stride_x = proof_bytes;
    w.proof_l = m.ln; w.proof_n = m.ln + 32 * (size_t)nl;
    w.stride_l = w.stride_n = 32 * ((size_t)nl + nn);
    w.transcript_preloaded = 1;
    w.accept = accept; w.status = status; w.tstate = r.tstate; w.acc = r.acc; w.pfix = r.pfix; w.ys = ys.data(); w.tab = tab.data();
    w.msc = msc.data(); w.straus = straus.data(); w.fb = r.fb;
    if (prev_ks) { m.ks = prev_ks; phase1_all(m, n, G); }
    m.ks = ks;
    phase1_all(m, n, G);
    for (size_t t = 0; t < n; t++) out_p1_status[t] = status[t];
    memcpy(out_sc0, sc0.data(), sc0.size() * sizeof(u32));
    memcpy(out_pts, pts.data(), pts.size() * sizeof(u32));
    memcpy(out_ln, ln.data(), ln.size());
    memcpy(out_einv, inv.data(), 8 * n * sizeof(u32));
    for (size_t t = 0; t < n; t++) {      // the uniform fixed-base half: 1 + k_max nd bases, zero scalars behind k_t nd
        pt a;
        FbRanges rg;
        agg_c0_fixed_ranges(rg, r);
        fb_sum_serial(a, r.fb, t, r.sc0, rg, nl_fixed);
        agg_c0_fixed_store(r, t, a);
    }
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
    if (r.atab) for (size_t t = 0; t < n; t++) agg_mixed_c0_tables(m, t);
    for (size_t t = 0; t < n; t++) agg_mixed_c0_var(m, t);
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

// The UNIFORM path (agg_core.h, one k for all) through phase 1 and the C0 stage on dense inputs (commitments n x k x 64, proofs
// n x proof_bytes(k)), for the word-for-word comparison with the mixed path on all-equal ks: sc0, pts, c (wn_c) and C0 (wn_commit).
int emul_agg_uniform_c0(const uint8_t* table, int W, int NG, int NH, int k, int nd, int np, const uint8_t* label, size_t label_len, size_t n,
                        const uint8_t* commitments, const uint8_t* proofs, int rounds, int nl, int nn, int G, int slow, uint8_t* out_c,
                        uint8_t* out_c0, int32_t* status, u32* out_sc0, u32* out_pts) {
    const size_t nm = (size_t)k * nd;
    AggWs r;
    memset(&r, 0, sizeof r);
    r.N = n; r.k = k; r.nd = nd; r.np = np; r.rounds = rounds; r.nl = nl; r.nn = nn; r.NG = NG; r.NH = NH;
    r.proof_bytes = 64 * (4 + 2 * (size_t)rounds + k) + 32 * ((size_t)nl + nn);
    r.commitments = commitments; r.proofs = proofs; r.status = status;
    std::vector<u32> ts(52 * n), sc0((nm + 5 + k) * 8 * n), pts((size_t)(4 + k) * 16 * n), acc(30 * n), pf(30 * n), inv((size_t)np * 8 * n),
        vs((size_t)k * 40 * n);
    std::vector<uint8_t> rho(32 * n), mu(32 * n);
    std::vector<pt_slot> straus(n * 5 * BPPP_STRAUS_ENTRIES);
    r.tstate = ts.data(); r.sc0 = sc0.data(); r.pts = pts.data(); r.acc = acc.data(); r.pfix = pf.data(); r.inv = inv.data();
    r.vsum = vs.data(); r.straus = straus.data();
    r.wn_commit = out_c0; r.wn_c = out_c; r.wn_rho = rho.data(); r.wn_mu = mu.data();
    r.fb.table = (const apt_packed*)table; r.fb.W = W; r.fb.N = n;
    t_new(r.base, label, (u32)label_len);
    for (size_t t = 0; t < n; t++) {
        if (G <= 1) { agg_phase1(r, t); continue; }
        AggHead h;
        sc ps, musum, p, s;
        agg_phase1_head(r, t, h);
        sc_set_u32(ps, 0); sc_set_u32(musum, 0);
        for (int q = G - 1; q >= 0; q--) { agg_phase1_run(r, t, h, q, G, p, s); sc_add(ps, ps, p); sc_add(musum, musum, s); }
        agg_phase1_tail(r, t, h, ps, musum);
    }
    memcpy(out_sc0, sc0.data(), sc0.size() * sizeof(u32));
    memcpy(out_pts, pts.data(), pts.size() * sizeof(u32));
    for (size_t t = 0; t < n; t++) {
        pt a;
        FbRanges rg;
        agg_c0_fixed_ranges(rg, r);
        fb_sum_serial(a, r.fb, t, r.sc0, rg);
        agg_c0_fixed_store(r, t, a);
    }
    std::vector<apt_packed> atab;
    std::vector<u32> tscr;
    if (rounds != 0 && !slow) {
        const size_t npts = 2 * (size_t)rounds + 4 + k;
        atab.assign(npts * 16 * n, apt_packed());
        tscr.assign((size_t)BPPP_TSCR_PER_POINT * npts * 10 * n, 0u);
        r.atab = atab.data(); r.tscr = tscr.data(); r.atab_first = 2 * rounds * 16;
    }
    if (r.atab) for (size_t t = 0; t < n; t++) agg_c0_tables(r, t);
    for (size_t t = 0; t < n; t++) agg_c0_var(r, t);
    for (size_t t = 0; t < n; t++) agg_c0_finish(r, t);
    return 0;
}

// The fixed-base sum over bases 0 .. count - 1 of the table on scalar sets given as workspace words [count * 8][n] (what phase 1
// leaves in sc0), in the form of nl lanes per instance (1: one lane, 8, 64: a wavefront; fb_sum_serial walks the lanes one after the
// other and falls back to the complete law as the kernels do) -> n x 64 affine bytes, the identity as zeros.
int emul_agg_mixed_fixed_sum(const uint8_t* table, int W, size_t n, int count, const u32* sc0, int nl, uint8_t* out) {
    FbTable fb;
    memset(&fb, 0, sizeof fb);
    fb.table = (const apt_packed*)table; fb.W = W; fb.N = n;
    for (size_t t = 0; t < n; t++) {
        pt a;
        FbRanges rg;
        fb_ranges_one(rg, 0, 0, count);
        fb_sum_serial(a, fb, t, sc0, rg, nl);
        apt p;
        pt_to_affine(p, a);
        apt_to_xy64(out + 64 * t, p);
    }
    return 0;
}

}  // extern "C"
