// TEST-ONLY host emulation of the aggregated reciprocal range proof ON THE CALLER'S TRANSCRIPTS: the device code the _transcript entry
// points run (bp_pp_amd/csrc/agg_core.h: agg_phase1<true>, agg_prove_core.h: agg_prove_stage_r1<true>, agg_prove_export; then the
// generic stages with tio / divergent_positions set, and tio_export), compiled with g++ and run one "thread" after the other as
// tests/emul/agg_emul.cpp and aggprove_emul.cpp run the label forms.  A translation unit of its own
// (tests/emul/build_agg_transcript.py builds it); the fixed-base table it takes is the one bppp_emul.cpp's emul_fb_build makes.
// states: n_states x 203 (1 = shared, n = one per instance); states_out: n x 203.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../bp_pp_amd/csrc/plan_core.h"      // (before the device headers: field.h pulls <stdio.h> in inside its namespace in the host build)
#include "../../bp_pp_amd/csrc/agg_prove_core.h"

using namespace bppp;

extern "C" {

size_t emul_aggtx_draws(size_t k, size_t nd) { return agg_prove_draws(k, nd); }
// the position-group key of instance t's state (verify_ws.h): its byte position, or 0x100 for a state merlin cannot be in
unsigned emul_aggtx_position_key(const uint8_t* states, size_t n_states, size_t t) { return preloaded_position_key(states, n_states, t); }

// Aggregated reciprocal verify on pre-loaded transcripts, every stage in thread order (emul_agg_verify's stages and outputs).
int emul_aggtx_verify(const uint8_t* table, int W, int NG, int NH, int k, int nd, int np, const uint8_t* states, size_t n_states, size_t n,
                    const uint8_t* commitments, const uint8_t* proofs, int rounds, int nl, int nn, int G, int slow, uint8_t* out_rho,
                    uint8_t* out_mu, uint8_t* out_c, uint8_t* out_pn, uint8_t* out_c0, int32_t* out_p1_status, uint8_t* accept,
                    int32_t* status, uint8_t* states_out) {
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
    t_new(r.base, nullptr, 0);                    // (as the entry points: a flagged instance runs from it)
    r.tio.states = states; r.tio.n_states = n_states; r.tio.states_out = states_out;
    WnlaWs w;
    memset(&w, 0, sizeof w);
    w.N = n; w.ng = NG; w.nh = NH; w.rounds = rounds; w.nl = nl; w.nn = nn;
    w.base = r.base; w.tio = r.tio; w.divergent_positions = n_states != 1;
    w.commitments = r.wn_commit; w.c = r.wn_c; w.rho = r.wn_rho; w.mu = r.wn_mu;
    w.proof_r = proofs + 256; w.proof_x = proofs + 256 + 64 * (size_t)rounds; w.proof_l = proofs + 64 * (size_t)(4 + k) + 128 * (size_t)rounds;
    w.proof_n = w.proof_l + 32 * (size_t)nl;
    w.stride_r = w.stride_x = w.stride_l = w.stride_n = proof_bytes;
    w.transcript_preloaded = 1;
    w.accept = accept; w.status = status; w.tstate = r.tstate; w.acc = r.acc; w.pfix = r.pfix; w.ys = ys.data(); w.tab = tab.data();
    w.msc = msc.data(); w.straus = straus.data(); w.fb = r.fb;
    for (size_t t = 0; t < n; t++) {
        if (G <= 1) { agg_phase1<true>(r, t); continue; }
        AggHead h;
        sc ps, musum, p, m;
        agg_phase1_head<true>(r, t, h);
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
    for (size_t t = 0; t < n; t++) tio_export(w.tio, w.base, w.tstate, n, w.status, t);      // (k_generic_export_states)
    return 0;
}


static void witness_ws(AggProveWs& a, size_t n, int k, int nd, int np, const uint8_t* x, const uint8_t* s, uint8_t* digits, uint8_t* m,
                       int32_t* status, std::vector<int32_t>& rst, std::vector<u32>& vsc) {
    memset(&a, 0, sizeof a);
    a.N = n; a.k = k; a.nd = nd; a.np = np;
    recip_witness_shape(a.rw, (size_t)nd, (size_t)np);
    a.x = x; a.s = s; a.digits = digits; a.m = m; a.status = status;
    rst.assign(n * k, 7);
    vsc.assign(16 * n * k, 0xA5A5A5A5u);
    a.row_status = rst.data(); a.vsc = vsc.data();
}
// The whole prover on pre-loaded transcripts (emul_aggprove's stages); the advanced states last.
int emul_aggtx_prove(const uint8_t* table, int W, int NG, int NH, int k, int nd, int np, const uint8_t* states, size_t n_states, size_t n,
                  const uint8_t* x, const uint8_t* s, const uint8_t* rnd, uint8_t* proofs, uint8_t* commitments, int32_t* status,
                     uint8_t* states_out) {
    const size_t nv = nd + 1, nm = (size_t)k * nd, nl = (size_t)k * nv, rows = n * k, NB = 1 + (size_t)NG + NH, n_rnd = agg_prove_draws(k, nd);
    size_t rounds, nl_f, nn_f;
    wnla_proof_shape((size_t)NH, (size_t)NG, rounds, nl_f, nn_f);
    const size_t proof_bytes = 64 * (4 + 2 * rounds + k) + 32 * (nl_f + nn_f);
    AggProveWs a;
    std::vector<int32_t> rst;
    std::vector<u32> vsc;
    std::vector<uint8_t> digits(n * nm * 32), m(n * (size_t)np * 32), com(rows * 64), cpv(rows * nv * 32), cpsv(rows * 32), cpwr(n * nm * 32),
        cpvp(rows * 64), prR(rows * 64);
    witness_ws(a, n, k, nd, np, x, s, digits.data(), m.data(), status, rst, vsc);
    a.NG = NG; a.NH = NH; a.n_rnd = (int)n_rnd; a.rnd = rnd; a.commitments = com.data();
    std::vector<u32> ts(52 * n), inst((2 + (size_t)np) * 8 * n), scr((nm + np) * 8 * n), rsc(nv * 8 * rows), rpb(30 * rows), vpb(30 * rows),
        vsum((size_t)k * 50 * n);
    a.tstate = ts.data(); a.inst_vals = inst.data(); a.scr = scr.data(); a.rsc = rsc.data(); a.rpb = rpb.data(); a.vsum = vsum.data();
    a.cp_v = cpv.data(); a.cp_sv = cpsv.data(); a.cp_wr = cpwr.data(); a.cp_vpts = cpvp.data(); a.proof_R = prR.data();
    a.fb.table = (const apt_packed*)table; a.fb.W = W; a.fb.N = rows;
    t_new(a.base, nullptr, 0);
    a.tio.states = states; a.tio.n_states = n_states; a.tio.states_out = states_out; a.divergent_positions = n_states != 1;
    RecipCommitWs cw;
    memset(&cw, 0, sizeof cw);
    cw.N = rows; cw.NG = NG; cw.x = x; cw.s = s; cw.status = a.row_status; cw.msc = a.vsc; cw.pbuf = vpb.data(); cw.out = com.data(); cw.fb = a.fb;
    AggProveShape shp;
    agg_prove_shape_build(shp, (size_t)k, (size_t)nd, (size_t)np);
    CircuitProveWs p;
    memset(&p, 0, sizeof p);
    p.base = a.base; p.tio = a.tio; p.divergent_positions = a.divergent_positions;
    CircuitDev& cd = p.cd;
    cd.nm = (int)nm; cd.no = np; cd.k = k; cd.nl = (int)nl; cd.nv = (int)nv; cd.nw = (int)(2 * nm + np); cd.f_l = 1; cd.f_m = 0;
    cd.a_l = shp.al.data(); cd.a_m = shp.am.data(); cd.inst_vals = a.inst_vals;
    p.N = n; p.NG = NG; p.NH = NH; p.n_rnd = (int)(18 + nv + nm); p.rnd_stride = n_rnd * 32; p.part = shp.parts.data(); p.transcript_preloaded = 1;
    p.v_pts = a.cp_vpts; p.v = a.cp_v; p.s_v = a.cp_sv; p.w_l = a.digits; p.w_r = a.cp_wr; p.w_o = a.m; p.rnd = rnd + 32 * (size_t)k; p.status = status;
    std::vector<uint8_t> head(n * 256), wc(n * 64), wcv(n * (size_t)NH * 32), wrho(n * 32), wmu(n * 32), wlv(n * (size_t)NH * 32), wnv(n * (size_t)NG * 32);
    std::vector<u32> r9(4 * 72 * n), lv(6 * nv * 8 * n), nvv(4 * nm * 8 * n), lam(nl * 8 * n), muv(nm * 8 * n), coef((3 * nm + 3 * nv) * 8 * n), misc(64 * n),
        msc(3 * NB * 8 * n, 0), pb(90 * n);
    p.proof_head = head.data(); p.tstate = ts.data();
    p.ro = r9.data(); p.rl = p.ro + 72 * n; p.rr = p.ro + 144 * n; p.rs = p.ro + 216 * n;
    p.lo = lv.data(); p.ll = p.lo + nv * 8 * n; p.lr = p.lo + 2 * nv * 8 * n; p.ls = p.lo + 3 * nv * 8 * n; p.v1 = p.lo + 4 * nv * 8 * n;
    p.cl0 = p.lo + 5 * nv * 8 * n;
    p.no = nvv.data(); p.nl = p.no + nm * 8 * n; p.nr = p.no + 2 * nm * 8 * n; p.ns = p.no + 3 * nm * 8 * n;
    p.lamv = lam.data(); p.muv = muv.data(); p.coef = coef.data(); p.misc = misc.data(); p.msc = msc.data(); p.pbuf = pb.data();
    p.wn_commit = wc.data(); p.wn_c = wcv.data(); p.wn_rho = wrho.data(); p.wn_mu = wmu.data(); p.wn_l = wlv.data(); p.wn_n = wnv.data();
    p.fb = a.fb; p.fb.N = n;
    std::vector<uint8_t> pr(n * rounds * 64 + 1), px(n * rounds * 64 + 1), pl(n * nl_f * 32 + 1), pn(n * nn_f * 32 + 1);
    WnlaProveWs w;
    memset(&w, 0, sizeof w);
    w.N = n; w.ng = NG; w.nh = NH; w.nl = NH; w.nn = NG; w.rounds = (int)rounds; w.nl_f = (int)nl_f; w.nn_f = (int)nn_f;
    w.transcript_preloaded = 1;
    w.commitments = p.wn_commit; w.c = p.wn_c; w.rho = p.wn_rho; w.mu = p.wn_mu; w.l_in = p.wn_l; w.n_in = p.wn_n;
    w.proof_r = pr.data(); w.proof_x = px.data(); w.proof_l = pl.data(); w.proof_n = pn.data(); w.status = status;
    std::vector<u32> vl((size_t)(NH + 1) * 8 * n), vn((size_t)(NG + 1) * 8 * n), vc((size_t)NH * 8 * n), ch((size_t)NH * 8 * n),
        cg((size_t)(NG + 1) * 8 * n), prm(24 * n), cm(16 * n);
    w.tstate = p.tstate; w.vl = vl.data(); w.vn = vn.data(); w.vc = vc.data(); w.ch = ch.data(); w.cg = cg.data(); w.prm = prm.data();
    w.com = cm.data(); w.msc = p.msc; w.pbuf = p.pbuf; w.fb = p.fb; w.base = p.base; w.tio = p.tio; w.divergent_positions = p.divergent_positions;
    std::vector<pt_slot> wstraus(n * 2 * BPPP_STRAUS_ENTRIES);
    w.straus = wstraus.data();
    auto sum = [&](const FbTable& fb, size_t count, const FbRanges& rg, const u32* scal, u32* out) {
        for (size_t t = 0; t < count; t++) { pt acc; fb_sum_serial(acc, fb, t, scal, rg); ws_st_pt(out, count, t, acc); }
    };
    FbRanges rg;
    for (size_t t = 0; t < n; t++) agg_prove_witness(a, t);
    recip_commit_ranges(rg, cw);
    sum(a.fb, rows, rg, cw.msc, cw.pbuf);
    for (size_t r = 0; r < rows; r++) recip_commit_store(cw, r);
    for (size_t t = 0; t < n; t++) agg_prove_stage_r1<true>(a, t);
    agg_prove_pole_ranges(rg, a);
    sum(a.fb, rows, rg, a.rsc, a.rpb);
    for (size_t t = 0; t < n; t++) agg_prove_stage_r2(a, t);
    for (size_t t = 0; t < n; t++) circuit_prove_stage_a(p, t);
    cp_ranges(rg, p, false);
    for (int set = 0; set < 3; set++) sum(p.fb, n, rg, p.msc + (size_t)set * cp_set_words(p), p.pbuf + (size_t)set * 30 * n);
    for (size_t t = 0; t < n; t++) agg_prove_stage_b(p, t);
    {   // the timed rerun of the collect leaves every array as it was
        std::vector<u32> lam0 = lam, mu0 = muv, coef0 = coef;
        for (size_t t = 0; t < n; t++) agg_collect_again(p, t);
        if (lam0 != lam || mu0 != muv || coef0 != coef) return -3;
    }
    sum(p.fb, n, rg, p.msc, p.pbuf);
    for (size_t t = 0; t < n; t++) circuit_prove_stage_c(p, t);
    cp_ranges(rg, p, true);
    sum(p.fb, n, rg, p.msc, p.pbuf);
    for (size_t t = 0; t < n; t++) circuit_prove_stage_d(p, t);
    for (size_t t = 0; t < n; t++) wnla_prove_init(w, t);
    wnla_prove_msm_ranges(rg, w);
    for (int kk = 0; kk < (int)rounds; kk++) {
        for (size_t t = 0; t < n; t++) wnla_prove_round_scalars(w, t, kk);
        sum(w.fb, n, rg, w.msc, w.pbuf);
        { FbRanges rr; wnla_prove_msm_ranges(rr, w, kk); sum(w.fb, n, rr, w.msc + wp_set_words(w), w.pbuf + 30 * n); }
        for (size_t t = 0; t < n; t++) wnla_prove_round_fold(w, t, kk);
        if (kk == 0 && rounds > 1) sum(w.fb, n, rg, w.msc + 2 * wp_set_words(w), w.pbuf + 60 * n);
    }
    for (size_t t = 0; t < n; t++) wnla_prove_finish(w, t);
    ProofAssembleWs as;
    memset(&as, 0, sizeof as);
    as.N = n; as.proof_bytes = proof_bytes; as.nseg = 6; as.status = status; as.out = proofs;
    as.src[0] = head.data(); as.bytes[0] = 256;
    as.src[1] = pr.data(); as.bytes[1] = (u32)(rounds * 64);
    as.src[2] = px.data(); as.bytes[2] = (u32)(rounds * 64);
    as.src[3] = prR.data(); as.bytes[3] = (u32)(k * 64);
    as.src[4] = pl.data(); as.bytes[4] = (u32)(nl_f * 32);
    as.src[5] = pn.data(); as.bytes[5] = (u32)(nn_f * 32);
    for (size_t t = 0; t < n; t++) for (u32 wd = 0; wd < proof_bytes / 4; wd++) proof_assemble_word(as, t, wd);
    ProofAssembleWs ac;
    memset(&ac, 0, sizeof ac);
    ac.N = n; ac.proof_bytes = (size_t)k * 64; ac.nseg = 1; ac.status = status; ac.out = commitments;
    ac.src[0] = com.data(); ac.bytes[0] = (u32)(k * 64);
    for (size_t t = 0; t < n; t++) for (u32 wd = 0; wd < (u32)k * 16; wd++) proof_assemble_word(ac, t, wd);
    for (size_t t = 0; t < n; t++) agg_prove_export(a.tio, a.base, p.tstate, n, status, t);      // (k_aprove_export_states)
    return (int)proof_bytes;
}

}  // extern "C"
