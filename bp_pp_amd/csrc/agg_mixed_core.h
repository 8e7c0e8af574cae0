// Batched verify of aggregated reciprocal range proofs of MIXED value counts: instance t carries k_t = ks[t] values, 1 <= k_t <= k_max,
// and is verified as the uniform call with k = k_t on the same context verifies it (agg_core.h has the protocol and the closed forms).
// Slots are laid out by k_max: instance t's commitments are the first k_t of its k_max x 64 bytes, its proof the first
// proof_bytes(k_t) bytes of its proof_bytes(k_max) slot in the uniform layout for k_t; what lies behind them is never read.
//
// What depends on k_t is phase 1 (the loops over the values, the k_t nd entries of pn_tau, S) and the number of points of C0's
// variable-base half (4 + k_t).  The workspace is AggWs with k = k_max: sc0 = ps_tau | pn_tau[k_max nd] | 4 | k_max coefficients and
// pts = 4 + k_max points, of which phase 1 writes the entries behind k_t as zero scalars and identity points on every call (the
// workspace is reused).  So C0's fixed-base half is the uniform kernel over 1 + k_max nd bases -- zero scalars add nothing --,
// agg_c0_finish and the WNLA stage are the uniform ones, and the variable-base half walks this instance's 4 + k_t points only.
// The WNLA stage finds l and n at one offset for every instance: phase 1 copies their 32 (nl + nn) bytes to `ln` as they are.
//
// An instance whose ks[t] is outside [1, k_max] (the device form cannot refuse it on the host) is flagged ST_BAD_ENCODING and runs as
// a malformed k = 1 instance: identity points everywhere, nothing read outside its slot.
// The functions below are agg_core.h's with k_t in the place of w.k; agg_core.h itself stays what it is, and with it the uniform kernels.
#pragma once
#include "agg_core.h"

namespace bppp {

struct AggMixedWs {
    AggWs w;                         // k = k_max, proof_bytes = the slot's stride, commitments N x k_max x 64
    const uint8_t* ks;               // [N] value counts
    uint8_t* ln;                     // [N][32 (nl + nn)]: l | n of every instance, for the WNLA stage
};

// k_t, or 1 with `bad` set where ks[t] is not a value count of this call
HD int agg_mixed_k(const AggMixedWs& m, size_t t, bool& bad) {
    const int k = (int)m.ks[t];
    bad = k < 1 || k > m.w.k;
    return bad ? 1 : k;
}
HD void agg_mixed_phase1_head(const AggMixedWs& m, size_t t, int k, bool bad_k, AggHead& h) {
    const AggWs& w = m.w;
    const size_t N = w.N;
    const int nd = w.nd, np = w.np;
    int32_t status = ST_OK;
    const uint8_t* pv = w.commitments + (size_t)64 * w.k * t;
    const uint8_t* pp = w.proofs + w.proof_bytes * t;
    const uint8_t* pr = pp + 256 + (size_t)128 * w.rounds;
    apt CL, CR, CO, CS, zero_pt;
    fe_set_u32(zero_pt.x, 0); fe_set_u32(zero_pt.y, 0);
    bool ok = apt_from_xy64(CL, pp) & apt_from_xy64(CR, pp + 64) & apt_from_xy64(CO, pp + 128) & apt_from_xy64(CS, pp + 192);
    ok &= !bad_k;
#pragma nounroll
    for (int i = 0; i < k; i++) { apt P; ok &= apt_from_xy64(P, pv + 64 * i); ok &= apt_from_xy64(P, pr + 64 * i); }
    if (!ok) { status |= ST_BAD_ENCODING; CL = zero_pt; CR = zero_pt; CO = zero_pt; CS = zero_pt; }
    strobe tr = w.base;
    fe one_fe, prodz;
    fe_set_u32(one_fe, 1);
    prodz = one_fe;
#pragma nounroll
    for (int i = 0; i < k; i++) {
        apt V, R;
        (void)apt_from_xy64(V, pv + 64 * i);
        (void)apt_from_xy64(R, pr + 64 * i);
        if (!ok) { V = zero_pt; R = zero_pt; }
        app_point(tr, "reciprocal_commitment", V);
        pt s;
        pt_from_affine(s, V);
        pt_madd(s, s, R, apt_is_identity(R));
        ws_st_pt(w.vsum + (size_t)i * 40 * N, N, t, s);
        agg_st_fe(w.vsum + (size_t)(i * 40 + 30) * N, N, t, 0, prodz);      // the product BEFORE Z_i
        fe z = s.Z;
        fe_cmov(z, fe_is_zero(s.Z), one_fe);
        fe_mul(prodz, prodz, z);
    }
    sc e, rho, lambda, beta, delta, tau;
    bool cok = t_get_challenge(tr, "reciprocal_challenge", e);
    {
        fe zi_all;
        fe_inv(zi_all, prodz);
#pragma nounroll
        for (int i = k - 1; i >= 0; i--) {
            pt s;
            fe pre, zi, z;
            ws_ld_pt(s, w.vsum + (size_t)i * 40 * N, N, t);
            agg_ld_fe(pre, w.vsum + (size_t)(i * 40 + 30) * N, N, t, 0, 1);
            const bool id = fe_is_zero(s.Z);
            z = s.Z;
            fe_cmov(z, id, one_fe);
            fe_mul(zi, zi_all, pre);               // 1 / Z_i
            fe_mul(zi_all, zi_all, z);
            apt a;
            fe_mul(a.x, s.X, zi);
            fe_mul(a.y, s.Y, zi);
            fe_cmov(a.x, id, zero_pt.x);
            fe_cmov(a.y, id, zero_pt.y);
            ws_st_apt(w.pts, N, t, 4 + i, a);
        }
    }
    app_point(tr, "commitment_cl", CL);
    app_point(tr, "commitment_cr", CR);
    app_point(tr, "commitment_co", CO);
#pragma nounroll
    for (int i = 0; i < k; i++) {
        apt a;
        ws_ld_apt(a, w.pts, N, t, 4 + i);
        app_point(tr, "commitment_v", a);
    }
    cok &= t_get_challenge(tr, "circuit_rho", rho);
    cok &= t_get_challenge(tr, "circuit_lambda", lambda);
    cok &= t_get_challenge(tr, "circuit_beta", beta);
    cok &= t_get_challenge(tr, "circuit_delta", delta);
    app_point(tr, "commitment_cs", CS);
    cok &= t_get_challenge(tr, "circuit_tau", tau);
    if (!cok) {
        status |= ST_DEGENERATE;
        sc_set_u32(e, 1); sc_set_u32(rho, 1); sc_set_u32(lambda, 1); sc_set_u32(beta, 1); sc_set_u32(delta, 1); sc_set_u32(tau, 1);
    }
    ws_st_strobe(w.tstate, N, t, tr);
    ws_st_apt(w.pts, N, t, 0, CS); ws_st_apt(w.pts, N, t, 1, CO); ws_st_apt(w.pts, N, t, 2, CL); ws_st_apt(w.pts, N, t, 3, CR);
    sc mu, one;
    sc_set_u32(one, 1);
    sc_mul(mu, rho, rho);
    sc_to_be(w.wn_rho + 32 * t, rho);
    sc_to_be(w.wn_mu + 32 * t, mu);
    bool zero_inv = sc_is_zero(delta) | sc_is_zero(mu) | sc_is_zero(tau);
    sc prod, m_ = sc_is_zero(mu) ? one : mu, t_ = sc_is_zero(tau) ? one : tau;
    sc_mul(prod, m_, t_);
#pragma nounroll
    for (int j = 0; j < np; j++) {
        sc js, a;
        sc_set_u32(js, (u32)j);
        sc_add(a, e, js);
        if (sc_is_zero(a)) { zero_inv = true; a = one; }
        ws_st8(w.inv, N, t, j, prod.v);          // prefix product BEFORE a_j
        sc_mul(prod, prod, a);
    }
    if (zero_inv) status |= ST_DEGENERATE;
    sc inv;
    sc_inv(inv, prod);
#pragma nounroll
    for (int j = np - 1; j >= 0; j--) {
        sc js, a, pre, aj;
        sc_set_u32(js, (u32)j);
        sc_add(a, e, js);
        if (sc_is_zero(a)) a = one;
        ws_ld8(pre.v, w.inv, N, t, j);
        sc_mul(aj, inv, pre);                    // (e + j)^-1
        sc_mul(inv, inv, a);
        ws_st8(w.inv, N, t, j, aj.v);
    }
    sc mu_inv, tau_inv;
    sc_mul(mu_inv, inv, t_);
    sc_mul(tau_inv, inv, m_);
    sc tau2;
    sc_mul(tau2, tau, tau);
    // S = (sum_{d=1..nd} lambda^d) (sum_{i<k_t} lambda^(nv i))
    sc S, lam_nv, lp, s_d, s_i;
    lp = lambda;
    s_d = lambda;
#pragma nounroll
    for (int d = 1; d < nd; d++) { sc_mul(lp, lp, lambda); sc_add(s_d, s_d, lp); }
    sc_mul(lam_nv, lp, lambda);                  // lambda^(nd + 1)
    s_i = one;
    lp = one;
#pragma nounroll
    for (int i = 1; i < k; i++) { sc_mul(lp, lp, lam_nv); sc_add(s_i, s_i, lp); }
    sc_mul(S, s_d, s_i);
    h.e = e; h.lambda = lambda; h.beta = beta; h.delta = delta; h.tau = tau; h.mu = mu; h.mu_inv = mu_inv; h.tau_inv = tau_inv;
    h.tau2 = tau2; h.S = S; h.lam_nv = lam_nv; h.status = status;
}
// run q of G over this instance's k_t nd entries, as agg_phase1_run; then the run's share of the padding: pn_tau slots
// k_t nd .. k_max nd cut into G pieces, written as zero
HD void agg_mixed_phase1_run(const AggMixedWs& m, size_t t, int k, const AggHead& h, int q, int G, sc& ps, sc& musum) {
    const AggWs& w = m.w;
    const size_t N = w.N;
    const int nd = w.nd, nm = k * nd, nm_max = w.k * nd;
    const sc &lambda = h.lambda, &mu = h.mu, &mu_inv = h.mu_inv, &tau = h.tau, &tau2 = h.tau2, &S = h.S, &lam_nv = h.lam_nv;
    sc one, zero, t1, t2, tau_e, base_np;
    sc_set_u32(one, 1);
    sc_set_u32(zero, 0);
    sc_mul(tau_e, tau, h.e);
    sc_set_u32(ps, 0);
    sc_set_u32(musum, 0);
    sc_set_u32(base_np, (u32)w.np);
    const int seg = (nm + G - 1) / G, ja = q * seg < nm ? q * seg : nm, jb = ja + seg < nm ? ja + seg : nm;
    int vi = ja / nd, d = ja % nd;
    sc pw, lv, tlv, ll, mip, mp;
    sc_pow_u32(pw, base_np, (u32)d);
    sc_pow_u32(lv, lam_nv, (u32)vi);
    sc_mul(tlv, tau2, lv);
    sc_pow_u32(ll, lambda, (u32)(1 + d));
    sc_mul(ll, ll, lv);
    if (ja == 0) { mip = mu_inv; mp = mu; }
    else { sc_pow_u32(mip, mu_inv, (u32)ja + 1); sc_pow_u32(mp, mu, (u32)ja + 1); }
#pragma nounroll
    for (int j = ja; j < jb; j++) {
        sc pn;
        sc_mul(t1, tlv, pw);
        sc_sub(t2, S, ll);
        sc_mul(t2, t2, tau);
        sc_add(t1, t1, t2);
        sc_mul(pn, t1, mip);
        sc_add(pn, pn, tau_e);
        ws_st8(w.sc0, N, t, 1 + j, pn.v);
        sc_mul(t1, pn, pn); sc_mul(t1, t1, mp); sc_add(ps, ps, t1);
        sc_add(musum, musum, mp);
        sc_mul(mip, mip, mu_inv);
        sc_mul(mp, mp, mu);
        if (++d == nd) {                         // the next entry is digit 0 of the next value
            d = 0;
            pw = one;
            sc_mul(lv, lv, lam_nv);
            sc_mul(tlv, tau2, lv);
            sc_mul(ll, lv, lambda);
        } else {
            sc_mul(ll, ll, lambda);
            sc_mul(pw, pw, base_np);
        }
    }
    const int pad = nm_max - nm, zseg = (pad + G - 1) / G, za = nm + (q * zseg < pad ? q * zseg : pad), zb = za + zseg < nm_max ? za + zseg : nm_max;
#pragma nounroll
    for (int j = za; j < zb; j++) ws_st8(w.sc0, N, t, 1 + j, zero.v);
}
// as agg_phase1_tail with the variable-base slots where k_max puts them; the coefficients and points of values >= k_t as zero and
// identity; l | n copied for the WNLA stage
HD void agg_mixed_phase1_tail(const AggMixedWs& m, size_t t, int k, const AggHead& h, const sc& ps_sum, const sc& musum) {
    const AggWs& w = m.w;
    const size_t N = w.N;
    const int nd = w.nd, np = w.np, nv = nd + 1, nm = w.k * nd;
    const sc &lambda = h.lambda, &beta = h.beta, &delta = h.delta, &tau = h.tau, &tau2 = h.tau2, &tau_inv = h.tau_inv, &lam_nv = h.lam_nv;
    sc one, zero, t1, tau3, two_tau3, two_tau2_S, ps, lp;
    sc_set_u32(one, 1);
    sc_set_u32(zero, 0);
    sc_mul(tau3, tau2, tau);
    sc_mul(two_tau2_S, tau2, h.S);
    sc_add(two_tau2_S, two_tau2_S, two_tau2_S);
    sc_add(two_tau3, tau3, tau3);
    sc_mul(t1, two_tau3, musum);
    sc_sub(ps, ps_sum, t1);
    ws_st8(w.sc0, N, t, 0, ps.v);
    ws_st8(w.sc0, N, t, 1 + nm, tau_inv.v);
    sc_neg(t1, delta);
    ws_st8(w.sc0, N, t, 2 + nm, t1.v);
    ws_st8(w.sc0, N, t, 3 + nm, tau.v);
    sc_neg(t1, tau2);
    ws_st8(w.sc0, N, t, 4 + nm, t1.v);
    sc cf = two_tau3;
#pragma nounroll
    for (int i = 0; i < k; i++) { ws_st8(w.sc0, N, t, 5 + nm + i, cf.v); sc_mul(cf, cf, lam_nv); }
    apt zero_pt;
    fe_set_u32(zero_pt.x, 0); fe_set_u32(zero_pt.y, 0);
#pragma nounroll
    for (int i = k; i < w.k; i++) { ws_st8(w.sc0, N, t, 5 + nm + i, zero.v); ws_st_apt(w.pts, N, t, 4 + i, zero_pt); }
    uint8_t* cw = w.wn_c + (size_t)t * w.NH * 32;
    sc_to_be(cw, one);
    sc_mul(t1, beta, tau_inv);
    sc_to_be(cw + 32, t1);
    sc bt = beta;
#pragma nounroll
    for (int i = 2; i < 9; i++) { sc_mul(bt, bt, tau); sc_to_be(cw + (size_t)i * 32, bt); }
    lp = lambda;
#pragma nounroll
    for (int j = 0; j < nv; j++) {
        sc cl = zero;
        if (j < np) { sc ej; ws_ld8(ej.v, w.inv, N, t, j); sc_mul(cl, two_tau2_S, ej); }
        if (j < nd) sc_sub(cl, cl, lp);
        sc_to_be(cw + (size_t)(9 + j) * 32, cl);
        sc_mul(lp, lp, lambda);
    }
#pragma nounroll
    for (int i = 9 + nv; i < w.NH; i++) sc_to_be(cw + (size_t)i * 32, zero);
    // l | n: behind this instance's 4 + 2 rounds + k_t points
    const int lnb = 32 * (w.nl + w.nn);
    const uint8_t* src = w.proofs + w.proof_bytes * t + 64 * (size_t)(4 + k) + 128 * (size_t)w.rounds;
    uint8_t* dst = m.ln + (size_t)lnb * t;
#pragma nounroll
    for (int i = 0; i < lnb; i++) dst[i] = src[i];
    w.status[t] = h.status;
}
// what follows the head: run q of G, the runs' sums, the tail on lane 0.  q, G: lane q of the G consecutive lanes of instance t (every
// lane of a group must be active; they share k_t); G = 1: one lane
HD void agg_mixed_phase1_rest(const AggMixedWs& m, size_t t, int k, const AggHead& h, int q, int G) {
    sc ps, musum;
    agg_mixed_phase1_run(m, t, k, h, q, G, ps, musum);
#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
    if (G > 1) { sc_group_sum16(ps, G); sc_group_sum16(musum, G); }      // (behind the runs' loops: the group's lanes are together again)
#endif
    if (q == 0) agg_mixed_phase1_tail(m, t, k, h, ps, musum);
}
// The SPONGE POSITION inside the head depends on k_t: between two challenges the transcript takes k_t points, and the transcript code
// keeps the position in a scalar register (merlin.h: st_uniform).  Every challenge squeezes from position 0, so the head begins and
// ends at one position for every k_t, and so does everything behind it (the WNLA stage continues at the position the last challenge
// leaves).  The kernels therefore run the HEAD once per value count present in the wavefront (k_agg_mixed.hip) and the rest, which
// touches no transcript, with per-lane trip counts.  This is the host order (the emulation's).
HD void agg_mixed_phase1(const AggMixedWs& m, size_t t, int q = 0, int G = 1) {
    AggHead h;
    bool bad;
    const int k = agg_mixed_k(m, t, bad);
    agg_mixed_phase1_head(m, t, k, bad, h);
    agg_mixed_phase1_rest(m, t, k, h, q, G);
}
// C0's variable-base half over this instance's 4 + k_t points: the window tables ...
HD void agg_mixed_c0_tables(const AggMixedWs& m, size_t t) {
    const AggWs& w = m.w;
    bool bad;
    const int k = agg_mixed_k(m, t, bad);
    affine_tables_build(atab_of(w.atab, w.N, t) + w.atab_first, w.tscr, w.pts, w.N, t, 4 + k);
}
// ... and the sum in chunks of at most five (agg_c0_chunk reads its scalars behind the k_max nd entries of pn_tau, where they are)
HD void agg_mixed_c0_var(const AggMixedWs& m, size_t t) {
    const AggWs& w = m.w;
    const size_t N = w.N;
    bool bad;
    const int k = agg_mixed_k(m, t, bad);
    const int npts = 4 + k, s0 = 1 + w.k * w.nd;
    pt total;
    pt_set_identity(total);
    if (w.atab) {
#pragma nounroll
        for (int first = 0; first < npts; first += 5) {
            const int c = npts - first < 5 ? npts - first : 5;
            pt acc;
            switch (c) {
            case 5: agg_c0_chunk<5>(acc, w, t, first); break;
            case 4: agg_c0_chunk<4>(acc, w, t, first); break;
            case 3: agg_c0_chunk<3>(acc, w, t, first); break;
            case 2: agg_c0_chunk<2>(acc, w, t, first); break;
            default: agg_c0_chunk<1>(acc, w, t, first); break;
            }
            if (first == 0) total = acc;
            else pt_add(total, total, acc);
        }
        ws_st_pt(w.acc, N, t, total);
        return;
    }
    pt_slot* tbl = w.straus + t * (5 * BPPP_STRAUS_ENTRIES);
#pragma nounroll
    for (int first = 0; first < npts; first += 5) {
        const int c = npts - first < 5 ? npts - first : 5;
        glv_split rs[5];
#pragma nounroll
        for (int j = 0; j < c; j++) {
            apt P;
            ws_ld_apt(P, w.pts, N, t, first + j);
            straus_build_table(tbl + j * BPPP_STRAUS_ENTRIES, P);
            sc kk;
            ws_ld8(kk.v, w.sc0, N, t, s0 + first + j);
            glv_decompose(rs[j], kk);
        }
        pt acc;
        straus_msm_glv(acc, tbl, rs, c);
        pt_add(total, total, acc);
    }
    ws_st_pt(w.acc, N, t, total);
}

}  // namespace bppp
