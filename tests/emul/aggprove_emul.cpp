// TEST-ONLY host emulation of the aggregated reciprocal range proof PROVER's device code (bp_pp_amd/csrc/agg_prove_core.h, then the
// generic circuit and WNLA provers): the exact __host__ __device__ functions the kernels of k_aggprove.hip / k_gprove.hip call, compiled
// with g++ and run one "thread" after the other.  A translation unit of its own (tests/emul/build_aggprove.py builds it); the fixed-base
// table it takes is the one bppp_emul.cpp's emul_fb_build makes.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../bp_pp_amd/csrc/plan_core.h"      // (before the device headers: field.h pulls <stdio.h> in inside its namespace in the host build)
#include "../../bp_pp_amd/csrc/agg_prove_core.h"

using namespace bppp;

extern "C" {

size_t emul_aggprove_draws(size_t k, size_t nd) { return agg_prove_draws(k, nd); }
int emul_aggprove_shape_ok(size_t k, size_t nd, size_t np, size_t ng, size_t nh) { return agg_prove_shape_ok(k, nd, np, ng, nh) ? 1 : 0; }
int emul_values_shape_ok(size_t nd, size_t np) { return recip_values_shape_ok(nd, np) ? 1 : 0; }

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
// the witness stage alone: digits [n x k nd x 32], m [n x np x 32], status [n], row status [n k], commitment scalars x_i | s_i [n k x 2 x 32]
int emul_aggprove_witness(int k, int nd, int np, size_t n, const uint8_t* x, const uint8_t* s, uint8_t* digits, uint8_t* m, int32_t* status,
                          int32_t* row_status, uint8_t* scalars) {
    AggProveWs a;
    std::vector<int32_t> rst;
    std::vector<u32> vsc;
    witness_ws(a, n, k, nd, np, x, s, digits, m, status, rst, vsc);
    for (size_t t = 0; t < n; t++) agg_prove_witness(a, t);
    for (size_t r = 0; r < n * k; r++) {
        row_status[r] = rst[r];
        for (int slot = 0; slot < 2; slot++) { sc v; ws_ld8(v.v, a.vsc, n * k, r, slot); sc_to_be(scalars + (r * 2 + slot) * 32, v); }
    }
    return 0;
}

// lambda_vec, mu_vec and the six coefficient vectors twice: circuit_collect on the aggregate's EXPLICIT sparse pattern (make_circuit of
// tests/agg_cases.py written out densely with this e, column-compressed by circuit_host_build), and agg_collect's closed forms.
// out_walk / out_closed: (nl + nm + 3 nm + 3 nv) x 8 words each, lamv | muv | coef.  Returns the word count, < 0 on a failure.
int emul_aggprove_collect(int k, int nd, int np, const uint8_t lambda_be[32], const uint8_t mu_be[32], const uint8_t e_be[32], u32* out_walk,
                          u32* out_closed) {
    const size_t nv = nd + 1, nm = (size_t)k * nd, nl = (size_t)k * nv, nw = 2 * nm + np, nout = 3 * nm + 3 * nv;
    sc lambda, mu, e, one, zero, mu_inv;
    if (!sc_from_be(lambda, lambda_be) || !sc_from_be(mu, mu_be) || !sc_from_be(e, e_be)) return -1;
    sc_set_u32(one, 1);
    sc_set_u32(zero, 0);
    sc_inv(mu_inv, mu);
    std::vector<sc> inv(np);
    for (int j = 0; j < np; j++) { sc js, a; sc_set_u32(js, (u32)j); sc_add(a, e, js); sc_inv(a, a); sc_neg(inv[j], a); }
    std::vector<uint8_t> Wm(nm * nw * 32, 0), Wl(nl * nw * 32, 0), am(nm * 32, 0), al(nl * 32, 0);
    auto put = [&](std::vector<uint8_t>& W, size_t row, size_t col, const sc& v) { sc_to_be(&W[(row * nw + col) * 32], v); };
    sc neg_e, base_np;
    sc_neg(neg_e, e);
    sc_set_u32(base_np, (u32)np);
    for (size_t J = 0; J < nm; J++) { put(Wm, J, nm + J, neg_e); am[J * 32 + 31] = 1; }
    for (int i = 0; i < k; i++) {
        sc pw = one;
        for (int d = 0; d < nd; d++) {
            sc v;
            sc_neg(v, pw);
            put(Wl, (size_t)i * nv, (size_t)i * nd + d, v);
            sc_mul(pw, pw, base_np);
            const size_t row = (size_t)i * nv + 1 + d;
            for (size_t J = 0; J < nm; J++) if (J != (size_t)i * nd + d) put(Wl, row, nm + J, one);
            for (int j = 0; j < np; j++) put(Wl, row, 2 * nm + j, inv[j]);
        }
    }
    std::vector<int32_t> plo(nv, -1), pll(nv, -1), plr(nv, -1), pno(nm, -1);
    for (size_t j = 0; j < nv && j < (size_t)np; j++) pll[j] = (int32_t)j;
    const size_t dims[6] = {nm, (size_t)np, (size_t)k, nl, nv, nw};
    CircuitHostData hd;
    if (!circuit_host_build(hd, dims, Wm.data(), Wl.data(), am.data(), al.data(), plo.data(), pll.data(), plr.data(), pno.data())) return -2;
    hd.rl.push_back(0); hd.rm.push_back(0); hd.vl.resize(hd.vl.size() + 8); hd.vm.resize(hd.vm.size() + 8);
    CircuitDev cd;
    memset(&cd, 0, sizeof cd);
    cd.nm = (int)nm; cd.no = np; cd.k = k; cd.nl = (int)nl; cd.nv = (int)nv; cd.nw = (int)nw; cd.f_l = 1; cd.f_m = 0;
    cd.colptr_l = hd.cpl.data(); cd.rows_l = hd.rl.data(); cd.vals_l = hd.vl.data();
    cd.colptr_m = hd.cpm.data(); cd.rows_m = hd.rm.data(); cd.vals_m = hd.vm.data();
    cd.colmap = hd.colmap.data(); cd.a_l = hd.al.data(); cd.a_m = hd.am.data();
    sc lam_nv[2], mu_nv[2];
    circuit_collect(cd, out_walk, out_walk + nl * 8, out_walk + (nl + nm) * 8, 1, 0, lambda, mu, mu_inv, lam_nv[0], mu_nv[0]);
    // the closed forms read only the shape and the per-instance values
    std::vector<u32> inst((2 + (size_t)np) * 8, 0);
    ws_st8(inst.data(), 1, 0, 0, neg_e.v);
    for (int j = 0; j < np; j++) ws_st8(inst.data(), 1, 0, 1 + j, inv[j].v);
    CircuitDev ca;
    memset(&ca, 0, sizeof ca);
    ca.nm = (int)nm; ca.no = np; ca.k = k; ca.nl = (int)nl; ca.nv = (int)nv; ca.nw = (int)nw; ca.f_l = 1; ca.f_m = 0;
    ca.inst_vals = inst.data();
    agg_collect(ca, out_closed, out_closed + nl * 8, out_closed + (nl + nm) * 8, 1, 0, lambda, mu, mu_inv, lam_nv[1], mu_nv[1]);
    if (memcmp(lam_nv[0].v, lam_nv[1].v, 32) || memcmp(mu_nv[0].v, mu_nv[1].v, 32)) return -3;      // lambda^nv, mu^nv handed to stage B
    return (int)((nl + nm + nout) * 8);
}

// The whole prover, every stage in thread order as agg_prove_part launches them: witness -> value commitments (N k rows) -> r1 -> pole
// commitments (N k rows) -> r2 -> stage A -> stage B with the closed-form collect -> stages C, D -> the WNLA prover -> assembly.
// Returns the proof size, < 0 on a failure.
int emul_aggprove(const uint8_t* table, int W, int NG, int NH, int k, int nd, int np, const uint8_t* label, size_t label_len, size_t n,
                  const uint8_t* x, const uint8_t* s, const uint8_t* rnd, uint8_t* proofs, uint8_t* commitments, int32_t* status) {
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
    t_new(a.base, label, (u32)label_len);
    RecipCommitWs cw;
    memset(&cw, 0, sizeof cw);
    cw.N = rows; cw.NG = NG; cw.x = x; cw.s = s; cw.status = a.row_status; cw.msc = a.vsc; cw.pbuf = vpb.data(); cw.out = com.data(); cw.fb = a.fb;
    AggProveShape shp;
    agg_prove_shape_build(shp, (size_t)k, (size_t)nd, (size_t)np);
    CircuitProveWs p;
    memset(&p, 0, sizeof p);
    p.base = a.base;
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
    w.com = cm.data(); w.msc = p.msc; w.pbuf = p.pbuf; w.fb = p.fb; w.base = p.base;
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
    for (size_t t = 0; t < n; t++) agg_prove_stage_r1(a, t);
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
    return (int)proof_bytes;
}

}  // extern "C"
