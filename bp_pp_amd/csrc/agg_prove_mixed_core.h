// Batched PROVER of aggregated reciprocal range proofs of MIXED value counts: instance t has k_t = ks[t] values, 1 <= k_t <= k_max, and
// gets the bytes the uniform prover with k = k_t on the same context gives its first k_t values, blindings and draws (agg_prove_core.h
// has the protocol, the stages and the closed forms; agg_mixed_core.h is the verifier's side of the same call).  Every buffer is laid out
// by k_max, as the mixed verifier reads them:
//   x, s          N x k_max x 32           the first k_t are read
//   rnd           N x D(k_max) x 32        D = agg_prove_draws; instance t uses its first D(k_t) rows, rb_0 .. rb_{k_t-1} | 18 | nd + 1 | k_t nd
//   proofs        N x proof_bytes(k_max)   the first proof_bytes(k_t) bytes in the uniform layout for k_t, zero behind them
//   commitments   N x k_max x 64           the first k_t, zero behind them
//
// The workspace is the uniform prover's with k = k_max (AggProveWs, CircuitProveWs) and ks beside it.  What depends on k_t:
//   witness, r1, r2   written out below with k_t in the place of w.k: the loops over the values, and the rows t k_max + i of the two
//                     fixed-base sums over N k_max rows.  Rows i >= k_t get zero scalars and the instance's status on every call (the
//                     workspace is reused) without a read of x or s, so the uniform sum kernels (k_rprove_commit*, k_aprove_msm) leave
//                     the identity there: a zero scalar adds nothing, in the gathered and in the full-scan ("ct_prover") form alike.
//   stages A, B, C    the generic circuit prover's functions as they are, on a lane's own VIEW of the workspace (agg_prove_mixed_view):
//                     cd.k, cd.nm, cd.nl for k_t, the draws behind k_t, and the per-instance inputs whose stride is a multiple of k
//                     (v_pts, v, s_v, w_l, w_r) re-based so that the lane's row index t with ITS k lands on its k_max slot.  coef, muv
//                     and lamv are then indexed by the lane's own nm, consistently between B and C and inside allocations sized for
//                     k_max; the partition table and a_l, a_m of the k_max shape are prefixes of every smaller shape's.  The scalar
//                     sets are cleared in front of stage A and every fill writes nm_t entries, so the uniform k_cprove_msm over the
//                     k_max ranges sees zeros behind them; stage C zero-extends l and n to the context's sizes itself.
//   the assembly      R_0 .. R_{k_t-1} and l | n directly behind this instance's 4 + 2 rounds + k_t points, zero bytes behind that.
// The SPONGE POSITION inside r1 and stage B depends on k_t (k_t points go in between two challenges), and the transcript code keeps the
// position wave-uniform (merlin.h: st_uniform): a wavefront runs these two stages once per value count present in it -- r1's
// transcript part in a loop inside its kernel, stage B in one launch per value count (k_aggprove_mixed.hip says why).  Every challenge
// squeezes from position 0, so stages C, D and the WNLA prover see one position in every lane.
//
// Secrets: k_t is public (the proof's length says it); values, digits, blindings and draws stay where the uniform stages keep them --
// nothing here branches on or indexes by anything but k_t and the loop counters.
// A ks[t] outside [1, k_max] (the device form cannot refuse it on the host) flags the instance ST_BAD_ENCODING; it runs as a one-value
// instance on x = s = rb = 0 without reading its x or s slots, and its outputs are zeroed.
#pragma once
#include "agg_prove_core.h"

namespace bppp {

struct AggProveMixedWs {
    AggProveWs a;                    // k = k_max; rows of the fixed-base sums: t k_max + i
    const uint8_t* ks;               // [N] value counts
};
struct CircuitProveMixedWs {
    CircuitProveWs p;                // cd of the k_max shape; rnd = the instance's draws behind k_max rb's, stride D(k_max)
    const uint8_t* ks;
    int k_max;
};

// the argument rule of the mixed prove calls besides the NULL checks of the buffers (pure): the uniform prover's with k = k_max, a ks,
// and -- where ks can be read -- every 1 <= ks[i] <= k_max
inline bool agg_prove_mixed_args_ok(size_t ng, size_t nh, size_t n, size_t k_max, const uint8_t* ks, bool ks_on_device, size_t nd, size_t np) {
    if (!ks || !agg_prove_shape_ok(k_max, nd, np, ng, nh)) return false;
    if (ks_on_device) return true;
    for (size_t i = 0; i < n; i++)
        if (ks[i] == 0 || ks[i] > k_max) return false;
    return true;
}

// k_t, or 1 with `bad` set where ks[t] is not a value count of this call
HD int agg_prove_mixed_k(const uint8_t* ks, int k_max, size_t t, bool& bad) {
    const int k = (int)ks[t];
    bad = k < 1 || k > k_max;
    return bad ? 1 : k;
}

// agg_prove_witness over k_t values: digits and multiplicities over k_t nd entries of the instance's k_max nd slot, the status, the
// commitment scalars of rows t k_max + i -- zero for i >= k_t
HD int32_t agg_prove_mixed_witness(const AggProveMixedWs& m, size_t t) {
    const AggProveWs& w = m.a;
    bool bad_k;
    const int k = agg_prove_mixed_k(m.ks, w.k, t, bad_k);
    const int k_max = w.k, nd = w.nd, np = w.np, nm = k * nd;
    uint8_t* dig = w.digits + t * (size_t)k_max * nd * 32;
    sc zero;
    sc_set_u32(zero, 0);
    u32 bad = bad_k ? 1u : 0u, over = 0;
#pragma nounroll
    for (int i = 0; i < k; i++) {
        sc xs = zero, ss = zero;
        bool canonical = true, s_ok = true;
        if (!bad_k) {
            canonical = sc_from_be(xs, w.x + (t * (size_t)k_max + i) * 32);
            s_ok = sc_from_be(ss, w.s + (t * (size_t)k_max + i) * 32);
        }
        u32 v[8];
#pragma unroll
        for (int l = 0; l < 8; l++) v[l] = xs.v[l];
#pragma nounroll
        for (int d = 0; d < nd; d++) {
            sc dd;
            sc_set_u32(dd, rw_next_digit(v, w.rw));
            sc_to_be(dig + ((size_t)i * nd + d) * 32, dd);
        }
        u32 rest = 0;
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
            const uint8_t* b = dig + (size_t)j * 32 + 28;
            const u32 d = ((u32)b[0] << 24) | ((u32)b[1] << 16) | ((u32)b[2] << 8) | (u32)b[3];
            count += (u32)(d == (u32)val);
        }
        sc c;
        sc_set_u32(c, count);
        sc_to_be(mo + (size_t)val * 32, c);
    }
    const int32_t status = (bad ? RW_BAD_ENCODING : 0) | (over ? RW_OUT_OF_RANGE : 0);
    const u32 keep = status == 0 ? ~0u : 0u;
    const size_t rows = w.N * (size_t)k_max;
#pragma nounroll
    for (int i = 0; i < k_max; i++) {
        const size_t row = t * (size_t)k_max + i;
        sc xs = zero, ss = zero;
        if (i < k && !bad_k) {
            (void)sc_from_be(xs, w.x + row * 32);
            (void)sc_from_be(ss, w.s + row * 32);
#pragma unroll
            for (int l = 0; l < 8; l++) { xs.v[l] &= keep; ss.v[l] &= keep; }
        }
        ws_st8(w.vsc, rows, row, 0, xs.v);
        ws_st8(w.vsc, rows, row, 1, ss.v);
        w.row_status[row] = status;
    }
    w.status[t] = status;
    return status;
}

// agg_prove_stage_r1 (label form) over k_t values.  The transcript part -- k_t points, then e -- is the HEAD, run once per value count in
// the wavefront; the rest touches no transcript.
HD void agg_prove_mixed_r1_head(const AggProveMixedWs& m, size_t t, int k, int32_t& status, bool& ok, sc& e) {
    const AggProveWs& w = m.a;
    status = w.status[t];
    ok = true;
    strobe tr = w.base;
#pragma nounroll
    for (int i = 0; i < k; i++) {
        apt V;
        if (!apt_from_xy64(V, w.commitments + (t * (size_t)w.k + i) * 64)) { ok = false; fe_set_u32(V.x, 0); fe_set_u32(V.y, 0); }
        app_point(tr, "reciprocal_commitment", V);
    }
    if (!t_get_challenge(tr, "reciprocal_challenge", e)) { status |= ST_DEGENERATE; sc_set_u32(e, 1); }
    ws_st_strobe(w.tstate, w.N, t, tr);
}
HD void agg_prove_mixed_r1_rest(const AggProveMixedWs& m, size_t t, int k, bool bad_k, int32_t status, bool ok, const sc& e) {
    const AggProveWs& w = m.a;
    const size_t N = w.N, rows = N * (size_t)w.k;
    const int k_max = w.k, nd = w.nd, np = w.np, nm = k * nd, nv = nd + 1;
    sc one, zero;
    sc_set_u32(one, 1);
    sc_set_u32(zero, 0);
    const uint8_t* dig = w.digits + t * (size_t)k_max * nd * 32;
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
    ws_st8(w.inst_vals, N, t, 0, neg.v);
    int vi = k - 1, d = nd - 1;
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
            const size_t row = t * (size_t)k_max + vi;
            sc_to_be(w.cp_wr + (t * (size_t)k_max * nd + i) * 32, ai);
            sc_to_be(w.cp_v + (row * nv + 1 + d) * 32, ai);
            ws_st8(w.rsc, rows, row, 1 + d, ai.v);
            if (--d < 0) { d = nd - 1; vi--; }
        } else {
            sc_neg(ai, ai);
            ws_st8(w.inst_vals, N, t, 1 + (i - nm), ai.v);
        }
    }
#pragma nounroll
    for (int i = 0; i < k; i++) {
        const size_t row = t * (size_t)k_max + i;
        sc xs = zero, ss = zero, rb = zero, sv;
        if (!bad_k) {
            (void)sc_from_be(xs, w.x + row * 32);
            (void)sc_from_be(ss, w.s + row * 32);
            ok &= sc_from_be(rb, w.rnd + ((size_t)t * w.n_rnd + i) * 32);
        }
        ws_st8(w.rsc, rows, row, 0, rb.v);
        sc_to_be(w.cp_v + row * nv * 32, xs);
        sc_add(sv, ss, rb);
        sc_to_be(w.cp_sv + row * 32, sv);
    }
    // the pole rows no value of this instance has: zero scalars, so that the sum over N k_max rows leaves the identity there
#pragma nounroll
    for (int i = k; i < k_max; i++) {
        const size_t row = t * (size_t)k_max + i;
#pragma nounroll
        for (int j = 0; j < nv; j++) ws_st8(w.rsc, rows, row, j, zero.v);
    }
    if (!ok) status |= ST_BAD_ENCODING;
    w.status[t] = status;
}
// this is the host order (the emulation's)
HD void agg_prove_mixed_stage_r1(const AggProveMixedWs& m, size_t t) {
    bool bad_k, ok;
    const int k = agg_prove_mixed_k(m.ks, m.a.k, t, bad_k);
    int32_t status;
    sc e;
    agg_prove_mixed_r1_head(m, t, k, status, ok, e);
    agg_prove_mixed_r1_rest(m, t, k, bad_k, status, ok, e);
}

// agg_prove_stage_r2 over 2 k_t points; rpb, vsum, cp_vpts and proof_R laid out by k_max
HD void agg_prove_mixed_stage_r2(const AggProveMixedWs& m, size_t t) {
    const AggProveWs& w = m.a;
    const size_t N = w.N, rows = N * (size_t)w.k;
    bool bad_k;
    const int k = agg_prove_mixed_k(m.ks, w.k, t, bad_k), k_max = w.k;
    apt zero_pt;
    fe_set_u32(zero_pt.x, 0); fe_set_u32(zero_pt.y, 0);
    fe one_fe, prodz;
    fe_set_u32(one_fe, 1);
    prodz = one_fe;
#pragma nounroll
    for (int i = 0; i < k; i++) {
        pt R, S;
        apt V;
        ws_ld_pt(R, w.rpb, rows, t * (size_t)k_max + i);
        if (!apt_from_xy64(V, w.commitments + (t * (size_t)k_max + i) * 64)) V = zero_pt;
        pt_madd(S, R, V, apt_is_identity(V));
        agg_st_fe(w.vsum + (size_t)(i * 50 + 40) * N, N, t, 0, prodz);
        fe z = R.Z;
        fe_cmov(z, fe_is_zero(R.Z), one_fe);
        fe_mul(prodz, prodz, z);
        ws_st_pt(w.vsum + (size_t)i * 50 * N, N, t, S);
        agg_st_fe(w.vsum + (size_t)(i * 50 + 30) * N, N, t, 0, prodz);
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
        fe_mul(zi, zi_all, pre);
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
        apt_to_xy64(w.cp_vpts + (t * (size_t)k_max + i) * 64, a);
        ws_ld_pt(R, w.rpb, rows, t * (size_t)k_max + i);
        agg_ld_fe(pre, w.vsum + (size_t)(i * 50 + 40) * N, N, t, 0, 1);
        to_affine(a, R, pre);
        apt_to_xy64(w.proof_R + (t * (size_t)k_max + i) * 64, a);
    }
}

// Instance t's own view of the circuit prover's workspace: the shape of k values, and every input the stages index by t k ... moved
// forward by t (k_max - k) units, so that t k + i of the view is t k_max + i of the workspace.  Nothing is copied but the struct.
HD CircuitProveWs agg_prove_mixed_view(const CircuitProveMixedWs& m, size_t t, int k) {
    CircuitProveWs v = m.p;
    const int nv = v.cd.nv, nd = nv - 1, gap = m.k_max - k;
    const size_t skip = t * (size_t)gap;
    v.cd.k = k;
    v.cd.nm = k * nd;
    v.cd.nl = k * nv;
    v.cd.nw = 2 * k * nd + v.cd.no;
    v.n_rnd = 18 + nv + k * nd;
    v.rnd = m.p.rnd - 32 * (size_t)gap;          // (m.p.rnd stands behind k_max rb's; this instance drew k of them)
    v.v_pts = m.p.v_pts + skip * 64;
    v.v = m.p.v + skip * (size_t)nv * 32;
    v.s_v = m.p.s_v + skip * 32;
    v.w_l = m.p.w_l + skip * (size_t)nd * 32;
    v.w_r = m.p.w_r + skip * (size_t)nd * 32;
    return v;
}
HD int agg_prove_mixed_ck(const CircuitProveMixedWs& m, size_t t) {
    bool bad_k;
    return agg_prove_mixed_k(m.ks, m.k_max, t, bad_k);
}
HD void agg_prove_mixed_stage_a(const CircuitProveMixedWs& m, size_t t) {
    circuit_prove_stage_a(agg_prove_mixed_view(m, t, agg_prove_mixed_ck(m, t)), t);
}
HD void agg_prove_mixed_stage_b(const CircuitProveMixedWs& m, size_t t, int k) {
    agg_prove_stage_b(agg_prove_mixed_view(m, t, k), t);
}
HD void agg_prove_mixed_collect_again(const CircuitProveMixedWs& m, size_t t) {
    agg_collect_again(agg_prove_mixed_view(m, t, agg_prove_mixed_ck(m, t)), t);
}
HD void agg_prove_mixed_stage_c(const CircuitProveMixedWs& m, size_t t) {
    circuit_prove_stage_c(agg_prove_mixed_view(m, t, agg_prove_mixed_ck(m, t)), t);
}

// The outputs put together on the device: ProofAssembleWs's pieces with piece `vseg` holding k_max x 64 bytes per instance of which
// the first k_t x 64 are taken; what follows them moves up, and the slot is zero behind the last piece.  A flagged instance gets zero
// bytes.  One 4-byte word of the slot per thread.
struct ProofAssembleMixedWs {
    ProofAssembleWs w;               // proof_bytes: the slot's stride; bytes[vseg] = k_max * 64
    const uint8_t* ks;
    int k_max, vseg;
};
HD void proof_assemble_mixed_word(const ProofAssembleMixedWs& m, size_t t, u32 word) {
    const ProofAssembleWs& w = m.w;
    bool bad_k;
    const int k = agg_prove_mixed_k(m.ks, m.k_max, t, bad_k);
    u32 off = 4 * word, v = 0;
    bool found = false;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        if (i < w.nseg && !found) {
            const u32 used = i == m.vseg ? 64u * (u32)k : w.bytes[i];
            if (off < used) { v = *(const u32*)(w.src[i] + t * (size_t)w.bytes[i] + off); found = true; }
            else off -= used;
        }
    }
    if (w.status[t] != ST_OK) v = 0;
    uint8_t* o = w.out + t * w.proof_bytes + 4 * (size_t)word;
    if ((((uintptr_t)o) & 3u) == 0) *(u32*)o = v;
    else { o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); o[3] = (uint8_t)(v >> 24); }
}

}  // namespace bppp
