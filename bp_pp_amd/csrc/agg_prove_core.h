// Batched PROVER of the aggregated reciprocal range proof: k values of dim_nd base-dim_np digits under one proof, from the integers
// (agg_core.h has the verifier and the circuit; tests/agg_cases.py::prove states the protocol on the oracle).  Per instance:
//   transcript = Transcript::new(label), or the caller's own (AggProveWs::tio); app_point("reciprocal_commitment", V_i) for i < k; e = challenge("reciprocal_challenge");
//   r_{i,d} = (digit_{i,d} + e)^-1;  R_i = rb_i h_vec[0] + sum_d r_{i,d} h_vec[9 + d];
//   ArithmeticCircuit::prove over the k commitments V_i + R_i with v_i = [x_i, r_i...], s_v[i] = s_i + rb_i, w_l = all digits
//   (value-major), w_r = all reciprocals, w_o = the multiplicities over all k nd digits.
// Draws per instance, in order: rb_0 .. rb_{k-1}, then the circuit prover's 18 + (nd + 1) + k nd (circuit_prove_core.h).
// Proof layout (the verifier's): c_l c_r c_o c_s | r | x | R_0 .. R_{k-1} | l | n;  commitments k x 64, value-major.
//
// Stages (each a kernel of k_aggprove.hip, a lane per instance unless said otherwise):
//   witness   digits and multiplicities of the k values (recip_witness_core.h's per-value routine, k times), the instance's status,
//             the scalars of the k value commitments -- rows t k + i of a fixed-base sum over N k rows (RecipCommitWs, k_rprove_commit)
//   r1        transcript to e, all k nd + np inversions from ONE sc_inv, -e and -(e + j)^-1, the circuit prover's inputs, the scalars
//             of the k pole commitments (rows again)
//   msm       R_i over N k rows (BPPP_FB_LANES lanes per row)
//   r2        R_i and V_i + R_i to affine with one field inversion over running products
//   then the generic circuit prover's stages with agg_collect below in place of circuit_collect's pattern walk, and the WNLA prover.
//
// The circuit's coefficient vectors in closed form (make_circuit of tests/agg_cases.py through collect_c, as pn_tau / cl_tau of
// agg_core.h): nv = nd + 1, nm = k nd, J = i nd + d, l(i, d) = lambda^(i nv + 1 + d), S = sum l(i, d):
//   c_nL[J] = -np^d lambda^(i nv) mu^-(J+1)      c_nR[J] = (S - l(i, d)) mu^-(J+1) + e      c_nO = 0
//   c_lL[j] = -S (e + j)^-1 for j < np, else 0   c_lR = c_lO = 0      lambda_vec[i] = lambda^i (f_l, not f_m)      mu_vec[j] = mu^(j+1)
// O(nm + nv + np) multiplications where the walk over W_l's dense nm x nm block of ones takes O(nm^2).
#pragma once
#include "agg_core.h"
#include "recip_prove_core.h"

namespace bppp {

// ---- argument rules (pure: the entry points and the CPU tier share them)
// draws per instance: rb_i (k) | ro, rl, rr (18) | ls (nv = nd + 1) | ns (nm = k nd)
inline size_t agg_prove_draws(size_t k, size_t nd) { return k + 18 + (nd + 1) + k * nd; }
// the verifier's conditions on a context with ng entries of g_vec and nh of h_vec, and dim_np^dim_nd <= n: x must determine its digits
inline bool agg_prove_shape_ok(size_t k, size_t nd, size_t np, size_t ng, size_t nh) {
    if (k == 0 || k > 64 || nd == 0 || np == 0 || nd > ng || k * nd > ng || nd + 10 > nh || np > nd + 1) return false;
    return recip_values_shape_ok(nd, np);
}

struct AggProveWs {
    size_t N;                  // instances; the fixed-base sums run over N k rows, row = t k + i
    int k, nd, np, NG, NH, n_rnd;
    RecipWitnessWs rw;         // the digit routine's shape fields (nd, np, bits, recip); nothing else of it is read
    const uint8_t *x, *s;      // N x k x 32, value-major
    const uint8_t* rnd;        // N x n_rnd x 32
    uint8_t* digits;           // N x k nd x 32: the circuit's w_l
    uint8_t* m;                // N x np x 32: the circuit's w_o
    int32_t* status;           // N
    int32_t* row_status;       // N k: the instance's witness status once per value (the commitment kernels flag by row)
    u32* vsc;                  // [2 * 8][N k]: x_i, s_i (zero in a flagged instance)
    const uint8_t* commitments;   // N x k x 64: V_i, as k_rprove_commit_store wrote them
    u32* tstate;               // [52][N]
    u32* inst_vals;            // [(2 + np) * 8][N]: -e, -(e + j)^-1, and mu^-1 (left by the collect for its timed rerun)
    u32* scr;                  // [(k nd + np) * 8][N]: prefix products of the batched inversion
    u32* rsc;                  // [(nd + 1) * 8][N k]: rb_i | r_{i,d}
    u32* rpb;                  // [30][N k]: R_i, projective
    u32* vsum;                 // [k * 50][N]: V_i + R_i (30) | the running product before its Z (10) | the one before R_i's Z (10)
    uint8_t *cp_v, *cp_sv, *cp_wr, *cp_vpts;   // the circuit prover's inputs: N x k x nv x 32, N x k x 32, N x k nd x 32, N x k x 64
    uint8_t* proof_R;          // N x k x 64
    FbTable fb;                // N = N k
    FbTable fb_ct;             // "ct_prover": the reciprocals and rb_i are secret
    int ct;
    strobe base;
    TranscriptIo tio;          // the caller's transcripts (the _transcript entry points); states null: Transcript::new(label)
    int divergent_positions;   // 1: the instances of one wavefront may sit at different sponge positions (per-instance input states)
};
HD void agg_prove_pole_ranges(FbRanges& rg, const AggProveWs& w) {
    rg.n = 2;
    rg.slot[0] = 0; rg.base[0] = 1 + w.NG; rg.count[0] = 1;                  // rb_i h_vec[0]
    rg.slot[1] = 1; rg.base[1] = 1 + w.NG + 9; rg.count[1] = w.nd;           // r_{i,d} h_vec[9 + d]
}

// digits (value-major), shared multiplicities, status; the scalars of the k value commitments.  Constant time in the values as
// recip_witness is: fixed-length loops, compare-and-accumulate, no branch or address that depends on a value or a digit.
HD int32_t agg_prove_witness(const AggProveWs& w, size_t t) {
    const int k = w.k, nd = w.nd, np = w.np, nm = k * nd;
    uint8_t* dig = w.digits + t * (size_t)nm * 32;
    u32 bad = 0, over = 0;
#pragma nounroll
    for (int i = 0; i < k; i++) {
        sc xs, ss;
        const bool canonical = sc_from_be(xs, w.x + (t * (size_t)k + i) * 32);
        const bool s_ok = sc_from_be(ss, w.s + (t * (size_t)k + i) * 32);
        u32 v[8];
#pragma unroll
        for (int l = 0; l < 8; l++) v[l] = xs.v[l];
#pragma nounroll
        for (int d = 0; d < nd; d++) {
            sc dd;
            sc_set_u32(dd, rw_next_digit(v, w.rw));
            sc_to_be(dig + ((size_t)i * nd + d) * 32, dd);
        }
        u32 rest = 0;      // what is left of x_i above its dim_nd digits: zero iff x_i < np^nd
#pragma unroll
        for (int l = 0; l < 8; l++) rest |= v[l];
        bad |= (u32)!canonical | (u32)!s_ok;
        over |= (u32)canonical & (u32)(rest != 0);
    }
    uint8_t* mo = w.m + t * (size_t)np * 32;
#pragma nounroll
    for (int val = 0; val < np; val++) {
        u32 count = 0;
#pragma nounroll
        for (int j = 0; j < nm; j++) {
            const uint8_t* b = dig + (size_t)j * 32 + 28;                       // (the address depends on j alone)
            const u32 d = ((u32)b[0] << 24) | ((u32)b[1] << 16) | ((u32)b[2] << 8) | (u32)b[3];
            count += (u32)(d == (u32)val);
        }
        sc c;
        sc_set_u32(c, count);
        sc_to_be(mo + (size_t)val * 32, c);
    }
    const int32_t status = (bad ? RW_BAD_ENCODING : 0) | (over ? RW_OUT_OF_RANGE : 0);
    const u32 keep = status == 0 ? ~0u : 0u;
    const size_t rows = w.N * (size_t)k;
#pragma nounroll
    for (int i = 0; i < k; i++) {
        const size_t row = t * (size_t)k + i;
        sc xs, ss;
        (void)sc_from_be(xs, w.x + row * 32);
        (void)sc_from_be(ss, w.s + row * 32);
#pragma unroll
        for (int l = 0; l < 8; l++) { xs.v[l] &= keep; ss.v[l] &= keep; }
        ws_st8(w.vsc, rows, row, 0, xs.v);
        ws_st8(w.vsc, rows, row, 1, ss.v);
        w.row_status[row] = status;
    }
    w.status[t] = status;
    return status;
}

// transcript over the k value commitments to e; reciprocals and the circuit's per-instance values from one inversion; the circuit
// prover's inputs; the scalar rows of the pole commitments
// TX: as agg_phase1_head's -- the label forms' kernel is the TX = false instantiation, `tr = w.base`
template <bool TX = false>
HD void agg_prove_stage_r1(const AggProveWs& w, size_t t) {
    const size_t N = w.N, rows = N * (size_t)w.k;
    const int k = w.k, nd = w.nd, np = w.np, nm = k * nd, nv = nd + 1;
    int32_t status = w.status[t];
    bool ok = true;
    sc one, e;
    sc_set_u32(one, 1);
    // TX: the caller's pre-loaded transcript; a state merlin cannot be in flags the instance: a zeroed proof, and its input state back
    strobe tr = w.base;
    if (TX) tio_begin(tr, status, w.tio, w.base, t);
#pragma nounroll
    for (int i = 0; i < k; i++) {
        apt V;
        if (!apt_from_xy64(V, w.commitments + (t * (size_t)k + i) * 64)) { ok = false; fe_set_u32(V.x, 0); fe_set_u32(V.y, 0); }
        app_point(tr, "reciprocal_commitment", V);
    }
    if (!t_get_challenge(tr, "reciprocal_challenge", e)) { status |= ST_DEGENERATE; e = one; }
    ws_st_strobe(w.tstate, N, t, tr);
    const uint8_t* dig = w.digits + t * (size_t)nm * 32;
    // one inversion for digit_J + e (J < nm) and e + j (j < np): prefix products forward, peel backwards
    bool zero_inv = false;
    sc prod = one;
#pragma nounroll
    for (int i = 0; i < nm + np; i++) {
        sc a;
        if (i < nm) { sc d; (void)sc_from_be(d, dig + (size_t)i * 32); sc_add(a, d, e); }
        else { sc js; sc_set_u32(js, (u32)(i - nm)); sc_add(a, e, js); }
        if (sc_is_zero(a)) { zero_inv = true; a = one; }
        ws_st8(w.scr, N, t, i, prod.v);
        sc_mul(prod, prod, a);
    }
    if (zero_inv) status |= ST_DEGENERATE;
    sc inv, neg;
    sc_inv(inv, prod);
    sc_neg(neg, e);
    ws_st8(w.inst_vals, N, t, 0, neg.v);                                      // W_m[J][nm + J] = -e
    int vi = k - 1, d = nd - 1;                                               // (value, digit) of entry i while i < nm
#pragma nounroll
    for (int i = nm + np - 1; i >= 0; i--) {
        sc a, pre, ai;
        if (i < nm) { sc dg; (void)sc_from_be(dg, dig + (size_t)i * 32); sc_add(a, dg, e); }
        else { sc js; sc_set_u32(js, (u32)(i - nm)); sc_add(a, e, js); }
        if (sc_is_zero(a)) a = one;
        ws_ld8(pre.v, w.scr, N, t, i);
        sc_mul(ai, inv, pre);
        sc_mul(inv, inv, a);
        if (i < nm) {
            const size_t row = t * (size_t)k + vi;
            sc_to_be(w.cp_wr + (t * (size_t)nm + i) * 32, ai);                // w_r = all reciprocals
            sc_to_be(w.cp_v + (row * nv + 1 + d) * 32, ai);                   // v_i = [x_i, r_i...]
            ws_st8(w.rsc, rows, row, 1 + d, ai.v);                            // R_i: h_vec[9 + d] r_{i,d}
            if (--d < 0) { d = nd - 1; vi--; }
        } else {
            sc_neg(ai, ai);
            ws_st8(w.inst_vals, N, t, 1 + (i - nm), ai.v);                    // W_l[i nv + 1 + d][2 nm + j] = -(e + j)^-1
        }
    }
#pragma nounroll
    for (int i = 0; i < k; i++) {
        const size_t row = t * (size_t)k + i;
        sc xs, ss, rb, sv;
        (void)sc_from_be(xs, w.x + row * 32);                                 // (the witness stage flagged a non-canonical x_i or s_i)
        (void)sc_from_be(ss, w.s + row * 32);
        ok &= sc_from_be(rb, w.rnd + ((size_t)t * w.n_rnd + i) * 32);
        ws_st8(w.rsc, rows, row, 0, rb.v);                                    // R_i: h_vec[0] rb_i
        sc_to_be(w.cp_v + row * nv * 32, xs);
        sc_add(sv, ss, rb);
        sc_to_be(w.cp_sv + row * 32, sv);                                     // s_v[i] = s_i + rb_i
    }
    if (!ok) status |= ST_BAD_ENCODING;
    w.status[t] = status;
}
// The caller's transcript after the prove: tio_export with every status bit in its mask -- an instance whose proof is zeroed (out of
// range, a non-canonical input, a degenerate challenge, an invalid state) gets its input state back: nothing was proved on it.
HD void agg_prove_export(const TranscriptIo& io, const strobe& base, const u32* tstate, size_t N, const int32_t* status, size_t t) {
    tio_export(io, base, tstate, N, status, t, ~0);
}
// R_i and V_i + R_i (the complete law: V_i = R_i, V_i = -R_i and identities included) to affine, 2 k points from one field inversion
HD void agg_prove_stage_r2(const AggProveWs& w, size_t t) {
    const size_t N = w.N, rows = N * (size_t)w.k;
    const int k = w.k;
    apt zero_pt;
    fe_set_u32(zero_pt.x, 0); fe_set_u32(zero_pt.y, 0);
    fe one_fe, prodz;
    fe_set_u32(one_fe, 1);
    prodz = one_fe;
#pragma nounroll
    for (int i = 0; i < k; i++) {
        pt R, S;
        apt V;
        ws_ld_pt(R, w.rpb, rows, t * (size_t)k + i);
        if (!apt_from_xy64(V, w.commitments + (t * (size_t)k + i) * 64)) V = zero_pt;
        pt_madd(S, R, V, apt_is_identity(V));
        agg_st_fe(w.vsum + (size_t)(i * 50 + 40) * N, N, t, 0, prodz);       // the product BEFORE Z(R_i)
        fe z = R.Z;
        fe_cmov(z, fe_is_zero(R.Z), one_fe);
        fe_mul(prodz, prodz, z);
        ws_st_pt(w.vsum + (size_t)i * 50 * N, N, t, S);
        agg_st_fe(w.vsum + (size_t)(i * 50 + 30) * N, N, t, 0, prodz);       // the product BEFORE Z(S_i)
        z = S.Z;
        fe_cmov(z, fe_is_zero(S.Z), one_fe);
        fe_mul(prodz, prodz, z);
    }
    fe zi_all;
    fe_inv(zi_all, prodz);
    auto to_affine = [&](apt& a, const pt& p, const fe& pre) {
        fe zi, z;
        const bool id = fe_is_zero(p.Z);
        z = p.Z;
        fe_cmov(z, id, one_fe);
        fe_mul(zi, zi_all, pre);                   // 1 / Z
        fe_mul(zi_all, zi_all, z);
        fe_mul(a.x, p.X, zi);
        fe_mul(a.y, p.Y, zi);
        fe_cmov(a.x, id, zero_pt.x);
        fe_cmov(a.y, id, zero_pt.y);
    };
#pragma nounroll
    for (int i = k - 1; i >= 0; i--) {
        pt R, S;
        fe pre;
        apt a;
        ws_ld_pt(S, w.vsum + (size_t)i * 50 * N, N, t);
        agg_ld_fe(pre, w.vsum + (size_t)(i * 50 + 30) * N, N, t, 0, 1);
        to_affine(a, S, pre);
        apt_to_xy64(w.cp_vpts + (t * (size_t)k + i) * 64, a);
        ws_ld_pt(R, w.rpb, rows, t * (size_t)k + i);
        agg_ld_fe(pre, w.vsum + (size_t)(i * 50 + 40) * N, N, t, 0, 1);
        to_affine(a, R, pre);
        apt_to_xy64(w.proof_R + (t * (size_t)k + i) * 64, a);
    }
}

// lambda_vec, mu_vec and the six coefficient vectors of the aggregate's circuit in closed form: what circuit_collect makes of the
// explicit pattern, word for word (tests/test_agg_prove_emul.py compares the two).  cd: nm = k nd, nv = nd + 1, no = np, f_l, and
// inst_vals = -e | -(e + j)^-1 | a slot for mu^-1; the pattern arrays are not read.
HD void agg_collect(const CircuitDev& cd, u32* lamv, u32* muv, u32* coef, size_t N, size_t t, const sc& lambda, const sc& mu, const sc& mu_inv,
                    sc& lam_nv, sc& mu_nv) {
    const int nm = cd.nm, nv = cd.nv, nd = nv - 1, nl = cd.nl, k = cd.k, np = cd.no;
    sc one, zero, e, t1;
    sc_set_u32(one, 1);
    sc_set_u32(zero, 0);
    ws_ld8(t1.v, cd.inst_vals, N, t, 0);
    sc_neg(e, t1);
    ws_st8(const_cast<u32*>(cd.inst_vals), N, t, 1 + np, mu_inv.v);
    sc lp = one;
#pragma nounroll
    for (int i = 0; i < nl; i++) { ws_st8(lamv, N, t, i, lp.v); sc_mul(lp, lp, lambda); }
    sc mp = mu;
#pragma nounroll
    for (int j = 0; j < nm; j++) { ws_st8(muv, N, t, j, mp.v); sc_mul(mp, mp, mu); }
    // S = (sum_{d=1..nd} lambda^d) (sum_{i<k} lambda^(nv i)), lambda^nv and mu^nv on the way
    sc S, s_d, s_i;
    lp = lambda;
    s_d = lambda;
    mu_nv = mu;
#pragma nounroll
    for (int d = 1; d < nd; d++) { sc_mul(lp, lp, lambda); sc_add(s_d, s_d, lp); sc_mul(mu_nv, mu_nv, mu); }
    sc_mul(lam_nv, lp, lambda);
    sc_mul(mu_nv, mu_nv, mu);
    s_i = one;
    lp = one;
#pragma nounroll
    for (int i = 1; i < k; i++) { sc_mul(lp, lp, lam_nv); sc_add(s_i, s_i, lp); }
    sc_mul(S, s_d, s_i);
    // the n-type vectors: J = i nd + d walked value by value
    sc base_np, pw = one, lv = one, ll = lambda, mip = mu_inv;      // np^d, lambda^(i nv), l(i, d), mu^-(J+1)
    sc_set_u32(base_np, (u32)np);
    int d = 0;
#pragma nounroll
    for (int J = 0; J < nm; J++) {
        sc cL, cR;
        sc_mul(t1, pw, lv);
        sc_mul(t1, t1, mip);
        sc_neg(cL, t1);
        sc_sub(t1, S, ll);
        sc_mul(t1, t1, mip);
        sc_add(cR, t1, e);
        ws_st8(coef, N, t, J, cL.v);
        ws_st8(coef, N, t, nm + J, cR.v);
        ws_st8(coef, N, t, 2 * nm + J, zero.v);
        sc_mul(mip, mip, mu_inv);
        if (++d == nd) {                           // the next entry is digit 0 of the next value
            d = 0;
            pw = one;
            sc_mul(lv, lv, lam_nv);
            sc_mul(ll, lv, lambda);
        } else {
            sc_mul(pw, pw, base_np);
            sc_mul(ll, ll, lambda);
        }
    }
    // the l-type vectors: c_lL[j] = S * (-(e + j)^-1) for j < np
#pragma nounroll
    for (int j = 0; j < nv; j++) {
        sc cL = zero;
        if (j < np) { ws_ld8(t1.v, cd.inst_vals, N, t, 1 + j); sc_mul(cL, S, t1); }
        ws_st8(coef, N, t, 3 * nm + j, cL.v);
        ws_st8(coef, N, t, 3 * nm + nv + j, zero.v);
        ws_st8(coef, N, t, 3 * nm + 2 * nv + j, zero.v);
    }
}
struct AggCollect {
    HD void operator()(const CircuitDev& cd, u32* lamv, u32* muv, u32* coef, size_t N, size_t t, const sc& lambda, const sc& mu, const sc& mu_inv,
                       sc& lam_nv, sc& mu_nv) const {
        agg_collect(cd, lamv, muv, coef, N, t, lambda, mu, mu_inv, lam_nv, mu_nv);
    }
};
// stage B of the circuit prover on the aggregate's circuit
HD void agg_prove_stage_b(const CircuitProveWs& w, size_t t) { circuit_prove_stage_b_with(w, t, AggCollect()); }
// the collect once more by itself from what stage B left (lambda, mu in misc; mu^-1 in inst_vals): same inputs, same outputs.  Run only
// when kernel timing is on, so that the collect's share of stage B can be read.
HD void agg_collect_again(const CircuitProveWs& w, size_t t) {
    sc lambda, mu, mu_inv, a, b;
    cp_ld(lambda, w.misc, w, t, CM_LAMBDA);
    cp_ld(mu, w.misc, w, t, CM_MU);
    ws_ld8(mu_inv.v, w.cd.inst_vals, w.N, t, 1 + w.cd.no);
    agg_collect(w.cd, w.lamv, w.muv, w.coef, w.N, t, lambda, mu, mu_inv, a, b);
}

// Host side: what of the aggregate's circuit the generic stages read besides the closed forms, for (k, dim_nd, dim_np):
// the partition tables LO | LL | LR | NO of stage A (LL & index < dim_np -> Some(index)), a_l = 0 and a_m = 1 of stage C.
struct AggProveShape {
    std::vector<int> parts;
    std::vector<u32> al, am;
};
inline void agg_prove_shape_build(AggProveShape& P, size_t k, size_t nd, size_t np) {
    const size_t nv = nd + 1, nm = k * nd, nl = k * nv;
    P.parts.assign(3 * nv + nm, -1);
    for (size_t j = 0; j < nv && j < np; j++) P.parts[nv + j] = (int)j;
    P.al.assign(nl * 8, 0);
    P.am.assign(nm * 8, 0);
    for (size_t i = 0; i < nm; i++) P.am[i * 8] = 1;
}

}  // namespace bppp
