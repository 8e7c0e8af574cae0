// Batched verify of the AGGREGATED reciprocal range proof: k values under one proof.  The circuit is the reciprocal circuit
// (reciprocal.rs:150-214) written for k values that share one multiplicity vector, verified by ArithmeticCircuit::verify with k
// commitments (circuit.rs:154-256); tests/agg_cases.py states it on the oracle.  nv = nd + 1, nm = k nd, J = i nd + d (value i, digit d).
//
// Transcript: app_point("reciprocal_commitment", V_i) for i < k | e | circuit.verify([V_i + R_i], t, circuit_proof), on
// Transcript::new(label) or on the caller's own transcript (AggWs::tio, as the other generic verifiers: verify_ws.h).
// Proof layout (per instance, proof_bytes = 64 (4 + 2 rounds + k) + 32 (nl + nn)):
//   c_l, c_r, c_o, c_s | r[rounds] | x[rounds] | R_0 .. R_{k-1} | l[nl] | n[nn];   commitments: k x 64, value-major.
//
// make_circuit / collect_c collapse to closed forms as they do for one value (recip_core.h).  With l(i, d) = lambda^(i nv + 1 + d) and
// S = sum_{i,d} l(i, d) = (sum_{d=1..nd} lambda^d) (sum_{i<k} lambda^(nv i)):
//   pn_tau[J] = (tau^2 np^d lambda^(i nv) + tau (S - l(i, d))) mu^-(J+1) + tau e
//   ps_tau    = sum_J pn_tau[J]^2 mu^(J+1) - 2 tau^3 sum_J mu^(J+1)
//   cl_tau[j] = 2 tau^2 S (e + j)^-1 [j < np] - lambda^(j+1) [j < nd]      for j < nv (j = nd is non-zero when np = nd + 1)
//   C0 = ps_tau g + <g_vec, pn_tau> + tau^-1 c_s - delta c_o + tau c_l - tau^2 c_r + sum_i 2 tau^3 lambda^(nv i) (V_i + R_i)
// Everything behind C0 is the generic WNLA stage (wnla_core.h), as for the reciprocal and circuit verifiers.
#pragma once
#include "recip_core.h"

namespace bppp {

struct AggWs {
    size_t N;
    int k, nd, np, rounds, nl, nn;
    int NG, NH;                      // lengths of g_vec || g_vec_ and h_vec || h_vec_ (the WNLA generator vectors)
    size_t proof_bytes;
    const uint8_t* commitments;      // N x k x 64
    const uint8_t* proofs;           // N x proof_bytes
    int32_t* status;
    u32* tstate;                     // [52][N]
    u32* sc0;                        // [(1 + nm + 4 + k) * 8][N]: ps_tau | pn_tau[nm] | tau^-1, -delta, tau, -tau^2 | 2 tau^3 lambda^(nv i) (k)
    u32* pts;                        // [(4 + k) * 16][N] packed affine: c_s, c_o, c_l, c_r, V_0 + R_0 .. V_{k-1} + R_{k-1}
    u32* acc;                        // [30][N]
    u32* pfix;                       // [30][N]
    u32* inv;                        // [np * 8][N]: (e + j)^-1
    u32* vsum;                       // [k * 40][N]: the k sums V_i + R_i (projective, 30 words) and the running products of their Z (10)
    pt_slot* straus;                 // [N][5][9]
    // fast variable-base path: window tables of the 4 + k points behind the WNLA stage's round-point tables (entry-major, atab_of);
    // null = the projective-table Straus sum on `straus`
    apt_packed* atab;
    u32* tscr;
    int atab_first;
    // outputs for the WNLA stage (C-ABI layouts)
    uint8_t* wn_commit;              // N x 64
    uint8_t* wn_c;                   // N x NH x 32
    uint8_t* wn_rho;                 // N x 32
    uint8_t* wn_mu;                  // N x 32
    FbTable fb;                      // bases: 0 g | 1..NG g_vec||g_vec_ | NG+1.. h_vec||h_vec_
    strobe base;
    TranscriptIo tio;                // the caller's transcripts (the _transcript entry points); states null: Transcript::new(label)
};

HD void agg_st_fe(u32* base, size_t N, size_t t, int slot, const fe& a) {
#pragma unroll
    for (int i = 0; i < 10; i++) base[(size_t)(slot * 10 + i) * N + t] = a.v[i];
}
HD void agg_ld_fe(fe& a, const u32* base, size_t N, size_t t, int slot, int mag) {
#pragma unroll
    for (int i = 0; i < 10; i++) a.v[i] = base[(size_t)(slot * 10 + i) * N + t];
    FE_SETMAG(a, mag);
    (void)mag;
}
// Phase 1 in three pieces, so that G (2, 4 or 8) consecutive lanes can run it for instance t together as in recip_phase1: the HEAD
// (decode, the k sums, transcript, inversions, S) is done by all lanes alike -- identical values, identical stores; the loop over the
// k nd entries of pn_tau, almost the whole kernel at 16 x 16, is cut into G RUNS of consecutive entries; the TAIL belongs to lane 0.
// (The host emulation calls the pieces itself and adds the runs' sums where the device shuffles.)
struct AggHead { sc e, lambda, beta, delta, tau, mu, mu_inv, tau_inv, tau2, S, lam_nv; int32_t status; };
// TX: the instance's transcript begins through tio_begin (the caller's pre-loaded state, or `base` when there is none).  The label
// forms' kernels are the TX = false instantiation -- `tr = w.base`, the code they always were -- and the _transcript forms' kernels
// the TX = true one, so that the label path's registers and scratch do not pay for the 200-byte state tio_begin decodes.
template <bool TX = false>
HD void agg_phase1_head(const AggWs& w, size_t t, AggHead& h) {
    const size_t N = w.N;
    const int k = w.k, nd = w.nd, np = w.np;
    int32_t status = ST_OK;
    const uint8_t* pv = w.commitments + (size_t)64 * k * t;
    const uint8_t* pp = w.proofs + w.proof_bytes * t;
    const uint8_t* pr = pp + 256 + (size_t)128 * w.rounds;
    apt CL, CR, CO, CS, zero_pt;
    fe_set_u32(zero_pt.x, 0); fe_set_u32(zero_pt.y, 0);
    bool ok = apt_from_xy64(CL, pp) & apt_from_xy64(CR, pp + 64) & apt_from_xy64(CO, pp + 128) & apt_from_xy64(CS, pp + 192);
    // a malformed instance runs on harmless values (identity points everywhere); its status forces accept = 0
#pragma nounroll
    for (int i = 0; i < k; i++) { apt P; ok &= apt_from_xy64(P, pv + 64 * i); ok &= apt_from_xy64(P, pr + 64 * i); }
    if (!ok) { status |= ST_BAD_ENCODING; CL = zero_pt; CR = zero_pt; CO = zero_pt; CS = zero_pt; }
    // TX: the caller's pre-loaded transcript; a state merlin cannot be in flags the instance, which then runs from `base` and gets its
    // input state back (tio_export)
    strobe tr = w.base;
    if (TX) tio_begin(tr, status, w.tio, w.base, t);
    // V_i into the transcript; V_i + R_i by the complete law (V_i = R_i, V_i = -R_i and identities included), kept projective with the
    // running products of their Z: ONE field inversion brings all k to affine
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
    app_point(tr, "commitment_cl", CL);                                   // circuit.rs:155-159
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
    // inverses of mu, tau, e + j (j < np) with one Fn inversion: running products forward, peel backwards (values kept in HBM)
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
    // inv = (mu tau)^-1
    sc mu_inv, tau_inv;
    sc_mul(mu_inv, inv, t_);
    sc_mul(tau_inv, inv, m_);
    sc tau2;
    sc_mul(tau2, tau, tau);
    // S as the product of two short sums (nd + k multiplications, every lane for itself), lambda^nv on the way
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
// run q of G: entries [ja, jb) of the k nd -> pn_tau[ja .. jb) stored, the run's shares of sum pn_tau^2 mu^(J+1) and sum mu^(J+1) returned.
// A run may cross value boundaries: it starts its powers at the exponents of its first entry (value vi, digit d) and steps them across
// a boundary as the one-lane loop does.
HD void agg_phase1_run(const AggWs& w, size_t t, const AggHead& h, int q, int G, sc& ps, sc& musum) {
    const size_t N = w.N;
    const int nd = w.nd, nm = w.k * nd;
    const sc &lambda = h.lambda, &mu = h.mu, &mu_inv = h.mu_inv, &tau = h.tau, &tau2 = h.tau2, &S = h.S, &lam_nv = h.lam_nv;
    sc one, t1, t2, tau_e, base_np;
    sc_set_u32(one, 1);
    sc_mul(tau_e, tau, h.e);
    sc_set_u32(ps, 0);
    sc_set_u32(musum, 0);
    sc_set_u32(base_np, (u32)w.np);
    const int seg = (nm + G - 1) / G, ja = q * seg < nm ? q * seg : nm, jb = ja + seg < nm ? ja + seg : nm;
    int vi = ja / nd, d = ja % nd;
    // np^d, lambda^(nv vi), tau^2 lambda^(nv vi), l(vi, d), mu^-(J+1), mu^(J+1) at the run's first entry
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
}
// ps, musum: the sums over all runs
HD void agg_phase1_tail(const AggWs& w, size_t t, const AggHead& h, const sc& ps_sum, const sc& musum) {
    const size_t N = w.N;
    const int k = w.k, nd = w.nd, np = w.np, nv = nd + 1, nm = k * nd;
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
    // variable-base scalars: tau^-1 c_s - delta c_o + tau c_l - tau^2 c_r + sum_i 2 tau^3 lambda^(nv i) (V_i + R_i)
    ws_st8(w.sc0, N, t, 1 + nm, tau_inv.v);
    sc_neg(t1, delta);
    ws_st8(w.sc0, N, t, 2 + nm, t1.v);
    ws_st8(w.sc0, N, t, 3 + nm, tau.v);
    sc_neg(t1, tau2);
    ws_st8(w.sc0, N, t, 4 + nm, t1.v);
    sc cf = two_tau3;
#pragma nounroll
    for (int i = 0; i < k; i++) { ws_st8(w.sc0, N, t, 5 + nm + i, cf.v); sc_mul(cf, cf, lam_nv); }
    // c = cr_tau (9) || cl_tau (nv) || zeros up to NH       (dim_np <= dim_nd + 1 = nv is required by the host)
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
    w.status[t] = h.status;
}
// q, G: lane q of the G consecutive lanes of instance t (every lane of a group must be active); G = 1: the one-lane form
template <bool TX = false>
HD void agg_phase1(const AggWs& w, size_t t, int q = 0, int G = 1) {
    AggHead h;
    sc ps, musum;
    agg_phase1_head<TX>(w, t, h);
    agg_phase1_run(w, t, h, q, G, ps, musum);
#if defined(__HIPCC__) && defined(__HIP_DEVICE_COMPILE__)
    if (G > 1) { sc_group_sum16(ps, G); sc_group_sum16(musum, G); }
#endif
    if (q == 0) agg_phase1_tail(w, t, h, ps, musum);      // (what is left belongs to the instance: lane 0 of the group)
}
// C0 fixed-base half: ps_tau g + <g_vec, pn_tau>  (bases 0..nm of the table)
HD void agg_c0_fixed_ranges(FbRanges& rg, const AggWs& w) { fb_ranges_one(rg, 0, 0, 1 + w.k * w.nd); }
HD void agg_c0_fixed_store(const AggWs& w, size_t t, const pt& total) { ws_st_pt(w.pfix, w.N, t, total); }
// C0 variable-base half: the 4 + k points (c_s, c_o, c_l, c_r, V_i + R_i: w.pts) in chunks of at most five per shared-doubling pass,
// as circuit_c0_var walks its 4 + k.  Window tables 1P .. 16P of all of them first (fast path)
HD void agg_c0_tables(const AggWs& w, size_t t) {
    affine_tables_build(atab_of(w.atab, w.N, t) + w.atab_first, w.tscr, w.pts, w.N, t, 4 + w.k);
}
template <int M>
HD void agg_c0_chunk(pt& acc, const AggWs& w, size_t t, int first) {
    const size_t N = w.N;
    int pslot[M];
    glv_words<M> g;
#pragma unroll
    for (int j = 0; j < M; j++) {
        pslot[j] = first + j;
        sc kk;
        ws_ld8(kk.v, w.sc0, N, t, 1 + w.k * w.nd + first + j);
        glv_split sp;
        glv_decompose(sp, kk);
        glv_words_set<M>(g, j, sp);
    }
    straus_affine<M>(acc, atab_of(w.atab, N, t) + w.atab_first, pslot, g);
}
HD void agg_c0_var(const AggWs& w, size_t t) {
    const size_t N = w.N;
    const int npts = 4 + w.k, s0 = 1 + w.k * w.nd;
    pt total;
    pt_set_identity(total);
    if (w.atab) {
#pragma nounroll
        for (int first = 0; first < npts; first += 5) {
            const int m = npts - first < 5 ? npts - first : 5;
            pt acc;
            switch (m) {
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
        const int m = npts - first < 5 ? npts - first : 5;
        glv_split rs[5];
#pragma nounroll
        for (int j = 0; j < m; j++) {
            apt P;
            ws_ld_apt(P, w.pts, N, t, first + j);
            straus_build_table(tbl + j * BPPP_STRAUS_ENTRIES, P);
            sc kk;
            ws_ld8(kk.v, w.sc0, N, t, s0 + first + j);
            glv_decompose(rs[j], kk);
        }
        pt acc;
        straus_msm_glv(acc, tbl, rs, m);
        pt_add(total, total, acc);
    }
    ws_st_pt(w.acc, N, t, total);
}
HD void agg_c0_finish(const AggWs& w, size_t t) {
    pt a, f;
    ws_ld_pt(a, w.acc, w.N, t);
    ws_ld_pt(f, w.pfix, w.N, t);
    pt_add(a, a, f);
    apt c0;
    pt_to_affine(c0, a);
    apt_to_xy64(w.wn_commit + 64 * t, c0);
}

}  // namespace bppp
