// TEST-ONLY host emulation of the aggregated reciprocal range proof PROVER for MIXED value counts (bp_pp_amd/csrc/agg_prove_mixed_core.h,
// then the generic circuit and WNLA provers): the exact __host__ __device__ functions the kernels of k_aggprove_mixed.hip / k_aggprove.hip /
// k_gprove.hip call, compiled with g++ and run one "thread" after the other in the order agg_prove_mixed_part launches them.  A
// translation unit of its own (tests/emul/build_aggprove_mixed.py builds it); the fixed-base table it takes is the one bppp_emul.cpp's
// emul_fb_build makes.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../bp_pp_amd/csrc/plan_core.h"      // (before the device headers: field.h pulls <stdio.h> in inside its namespace in the host build)
#include "../../bp_pp_amd/csrc/agg_prove_mixed_core.h"

using namespace bppp;

extern "C" {

int emul_aggprove_mixed_args_ok(size_t ng, size_t nh, size_t n, size_t k_max, const uint8_t* ks, int ks_on_device, size_t nd, size_t np) {
    return agg_prove_mixed_args_ok(ng, nh, n, k_max, ks, ks_on_device != 0, nd, np) ? 1 : 0;
}

// The whole mixed prover on ONE workspace, once per input set: first (prev_ks, prev_x, prev_s, prev_rnd) when prev_ks is not NULL -- what
// the workspace was last used for --, then (ks, x, s, rnd), whose outputs and padding are returned.  Layouts by k = k_max.
//   msc_a   [3][(1 + NG + NH) * 8][n]   the scalar sets of c_o, c_l, c_r as the sums behind stage A read them
//   msc_b   [(1 + NG + NH) * 8][n]      the scalar set of c_s
//   wn_n    [n][NG][32]                 the WNLA witness n
//   vsc     [2 * 8][n k]                the value commitments' scalars by row;  rsc [(nd + 1) * 8][n k] the pole commitments'
// Returns the proof slot's size, < 0 on a failure.
int emul_aggprove_mixed(const uint8_t* table, int W, int NG, int NH, int k, int nd, int np, const uint8_t* label, size_t label_len, size_t n,
                        const uint8_t* ks, const uint8_t* x, const uint8_t* s, const uint8_t* rnd, const uint8_t* prev_ks, const uint8_t* prev_x,
                        const uint8_t* prev_s, const uint8_t* prev_rnd, uint8_t* proofs, uint8_t* commitments, int32_t* status, u32* msc_a,
                        u32* msc_b, uint8_t* wn_n_out, u32* vsc_out, u32* rsc_out) {
    const size_t nv = nd + 1, nm = (size_t)k * nd, nl = (size_t)k * nv, rows = n * k, NB = 1 + (size_t)NG + NH, n_rnd = agg_prove_draws(k, nd);
    size_t rounds, nl_f, nn_f;
    wnla_proof_shape((size_t)NH, (size_t)NG, rounds, nl_f, nn_f);
    const size_t proof_bytes = 64 * (4 + 2 * rounds + k) + 32 * (nl_f + nn_f);
    std::vector<int32_t> rst(rows, 7);
    std::vector<u32> vsc(16 * rows, 0xA5A5A5A5u);
    std::vector<uint8_t> digits(n * nm * 32, 0xEE), mul(n * (size_t)np * 32, 0xEE), com(rows * 64, 0xEE), cpv(rows * nv * 32, 0xEE), cpsv(rows * 32, 0xEE),
        cpwr(n * nm * 32, 0xEE), cpvp(rows * 64, 0xEE), prR(rows * 64, 0xEE);
    std::vector<u32> ts(52 * n), inst((2 + (size_t)np) * 8 * n), scr((nm + np) * 8 * n), rsc(nv * 8 * rows, 0xA5A5A5A5u), rpb(30 * rows), vpb(30 * rows),
        vsum((size_t)k * 50 * n);
    AggProveShape shp;
    agg_prove_shape_build(shp, (size_t)k, (size_t)nd, (size_t)np);
    std::vector<uint8_t> head(n * 256), wc(n * 64), wcv(n * (size_t)NH * 32), wrho(n * 32), wmu(n * 32), wlv(n * (size_t)NH * 32), wnv(n * (size_t)NG * 32);
    std::vector<u32> r9(4 * 72 * n), lv(6 * nv * 8 * n), nvv(4 * nm * 8 * n, 0xA5A5A5A5u), lam(nl * 8 * n), muv(nm * 8 * n),
        coef((3 * nm + 3 * nv) * 8 * n), misc(64 * n), msc(3 * NB * 8 * n, 0), pb(90 * n);
    std::vector<uint8_t> pr(n * rounds * 64 + 1), px(n * rounds * 64 + 1), pl(n * nl_f * 32 + 1), pn(n * nn_f * 32 + 1);
    std::vector<u32> vl((size_t)(NH + 1) * 8 * n), vn((size_t)(NG + 1) * 8 * n), vc((size_t)NH * 8 * n), ch((size_t)NH * 8 * n),
        cg((size_t)(NG + 1) * 8 * n), prm(24 * n), cm(16 * n);
    std::vector<pt_slot> wstraus(n * 2 * BPPP_STRAUS_ENTRIES);

    auto chain = [&](const uint8_t* ks_, const uint8_t* x_, const uint8_t* s_, const uint8_t* rnd_) -> int {
        AggProveMixedWs am;
        memset(&am, 0, sizeof am);
        am.ks = ks_;
        AggProveWs& a = am.a;
        a.N = n; a.k = k; a.nd = nd; a.np = np;
        recip_witness_shape(a.rw, (size_t)nd, (size_t)np);
        a.x = x_; a.s = s_; a.digits = digits.data(); a.m = mul.data(); a.status = status;
        a.row_status = rst.data(); a.vsc = vsc.data();
        a.NG = NG; a.NH = NH; a.n_rnd = (int)n_rnd; a.rnd = rnd_; a.commitments = com.data();
        a.tstate = ts.data(); a.inst_vals = inst.data(); a.scr = scr.data(); a.rsc = rsc.data(); a.rpb = rpb.data(); a.vsum = vsum.data();
        a.cp_v = cpv.data(); a.cp_sv = cpsv.data(); a.cp_wr = cpwr.data(); a.cp_vpts = cpvp.data(); a.proof_R = prR.data();
        a.fb.table = (const apt_packed*)table; a.fb.W = W; a.fb.N = rows;
        t_new(a.base, label, (u32)label_len);
        RecipCommitWs cw;
        memset(&cw, 0, sizeof cw);
        cw.N = rows; cw.NG = NG; cw.x = x_; cw.s = s_; cw.status = a.row_status; cw.msc = a.vsc; cw.pbuf = vpb.data(); cw.out = com.data(); cw.fb = a.fb;
        CircuitProveMixedWs pm;
        memset(&pm, 0, sizeof pm);
        pm.ks = ks_; pm.k_max = k;
        CircuitProveWs& p = pm.p;
        p.base = a.base;
        CircuitDev& cd = p.cd;
        cd.nm = (int)nm; cd.no = np; cd.k = k; cd.nl = (int)nl; cd.nv = (int)nv; cd.nw = (int)(2 * nm + np); cd.f_l = 1; cd.f_m = 0;
        cd.a_l = shp.al.data(); cd.a_m = shp.am.data(); cd.inst_vals = a.inst_vals;
        p.N = n; p.NG = NG; p.NH = NH; p.n_rnd = (int)(18 + nv + nm); p.rnd_stride = n_rnd * 32; p.part = shp.parts.data(); p.transcript_preloaded = 1;
        p.v_pts = a.cp_vpts; p.v = a.cp_v; p.s_v = a.cp_sv; p.w_l = a.digits; p.w_r = a.cp_wr; p.w_o = a.m; p.rnd = rnd_ + 32 * (size_t)k; p.status = status;
        p.proof_head = head.data(); p.tstate = ts.data();
        p.ro = r9.data(); p.rl = p.ro + 72 * n; p.rr = p.ro + 144 * n; p.rs = p.ro + 216 * n;
        p.lo = lv.data(); p.ll = p.lo + nv * 8 * n; p.lr = p.lo + 2 * nv * 8 * n; p.ls = p.lo + 3 * nv * 8 * n; p.v1 = p.lo + 4 * nv * 8 * n;
        p.cl0 = p.lo + 5 * nv * 8 * n;
        p.no = nvv.data(); p.nl = p.no + nm * 8 * n; p.nr = p.no + 2 * nm * 8 * n; p.ns = p.no + 3 * nm * 8 * n;
        p.lamv = lam.data(); p.muv = muv.data(); p.coef = coef.data(); p.misc = misc.data(); p.msc = msc.data(); p.pbuf = pb.data();
        p.wn_commit = wc.data(); p.wn_c = wcv.data(); p.wn_rho = wrho.data(); p.wn_mu = wmu.data(); p.wn_l = wlv.data(); p.wn_n = wnv.data();
        p.fb = a.fb; p.fb.N = n;
        WnlaProveWs w;
        memset(&w, 0, sizeof w);
        w.N = n; w.ng = NG; w.nh = NH; w.nl = NH; w.nn = NG; w.rounds = (int)rounds; w.nl_f = (int)nl_f; w.nn_f = (int)nn_f;
        w.transcript_preloaded = 1;
        w.commitments = p.wn_commit; w.c = p.wn_c; w.rho = p.wn_rho; w.mu = p.wn_mu; w.l_in = p.wn_l; w.n_in = p.wn_n;
        w.proof_r = pr.data(); w.proof_x = px.data(); w.proof_l = pl.data(); w.proof_n = pn.data(); w.status = status;
        w.tstate = p.tstate; w.vl = vl.data(); w.vn = vn.data(); w.vc = vc.data(); w.ch = ch.data(); w.cg = cg.data(); w.prm = prm.data();
        w.com = cm.data(); w.msc = p.msc; w.pbuf = p.pbuf; w.fb = p.fb; w.base = p.base;
        w.straus = wstraus.data();
        auto sum = [&](const FbTable& fb, size_t count, const FbRanges& rg, const u32* scal, u32* out) {
            for (size_t t = 0; t < count; t++) { pt acc; fb_sum_serial(acc, fb, t, scal, rg); ws_st_pt(out, count, t, acc); }
        };
        FbRanges rg;
        for (size_t t = 0; t < n; t++) agg_prove_mixed_witness(am, t);
        recip_commit_ranges(rg, cw);
        sum(a.fb, rows, rg, cw.msc, cw.pbuf);
        for (size_t r = 0; r < rows; r++) recip_commit_store(cw, r);
        for (size_t t = 0; t < n; t++) agg_prove_mixed_stage_r1(am, t);
        agg_prove_pole_ranges(rg, a);
        sum(a.fb, rows, rg, a.rsc, a.rpb);
        for (size_t t = 0; t < n; t++) agg_prove_mixed_stage_r2(am, t);
        std::fill(msc.begin(), msc.end(), 0u);                                    // (the host's hipMemsetAsync in front of stage A)
        for (size_t t = 0; t < n; t++) agg_prove_mixed_stage_a(pm, t);
        memcpy(msc_a, msc.data(), 3 * NB * 8 * n * 4);
        cp_ranges(rg, p, false);
        for (int set = 0; set < 3; set++) sum(p.fb, n, rg, p.msc + (size_t)set * cp_set_words(p), p.pbuf + (size_t)set * 30 * n);
        for (size_t t = 0; t < n; t++) agg_prove_mixed_stage_b(pm, t, agg_prove_mixed_ck(pm, t));
        memcpy(msc_b, msc.data(), NB * 8 * n * 4);
        {   // the timed rerun of the collect leaves every array as it was
            std::vector<u32> lam0 = lam, mu0 = muv, coef0 = coef;
            for (size_t t = 0; t < n; t++) agg_prove_mixed_collect_again(pm, t);
            if (lam0 != lam || mu0 != muv || coef0 != coef) return -3;
        }
        sum(p.fb, n, rg, p.msc, p.pbuf);
        for (size_t t = 0; t < n; t++) agg_prove_mixed_stage_c(pm, t);
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
        ProofAssembleMixedWs as;
        memset(&as, 0, sizeof as);
        as.ks = ks_; as.k_max = k; as.vseg = 3;
        as.w.N = n; as.w.proof_bytes = proof_bytes; as.w.nseg = 6; as.w.status = status; as.w.out = proofs;
        as.w.src[0] = head.data(); as.w.bytes[0] = 256;
        as.w.src[1] = pr.data(); as.w.bytes[1] = (u32)(rounds * 64);
        as.w.src[2] = px.data(); as.w.bytes[2] = (u32)(rounds * 64);
        as.w.src[3] = prR.data(); as.w.bytes[3] = (u32)(k * 64);
        as.w.src[4] = pl.data(); as.w.bytes[4] = (u32)(nl_f * 32);
        as.w.src[5] = pn.data(); as.w.bytes[5] = (u32)(nn_f * 32);
        for (size_t t = 0; t < n; t++) for (u32 wd = 0; wd < proof_bytes / 4; wd++) proof_assemble_mixed_word(as, t, wd);
        ProofAssembleMixedWs ac;
        memset(&ac, 0, sizeof ac);
        ac.ks = ks_; ac.k_max = k; ac.vseg = 0;
        ac.w.N = n; ac.w.proof_bytes = (size_t)k * 64; ac.w.nseg = 1; ac.w.status = status; ac.w.out = commitments;
        ac.w.src[0] = com.data(); ac.w.bytes[0] = (u32)(k * 64);
        for (size_t t = 0; t < n; t++) for (u32 wd = 0; wd < (u32)k * 16; wd++) proof_assemble_mixed_word(ac, t, wd);
        return 0;
    };
    if (prev_ks) { const int rc = chain(prev_ks, prev_x, prev_s, prev_rnd); if (rc) return rc; }
    const int rc = chain(ks, x, s, rnd);
    if (rc) return rc;
    memcpy(wn_n_out, wnv.data(), wnv.size());
    memcpy(vsc_out, vsc.data(), vsc.size() * 4);
    memcpy(rsc_out, rsc.data(), rsc.size() * 4);
    return (int)proof_bytes;
}

}  // extern "C"
