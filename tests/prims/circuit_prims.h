// TEST-ONLY: what the two builds of the circuit-stage entry point share (prims_host.cpp: prims_run_circuit_host, the single-thread form
// of circuit_core.h as tests/emul runs it; circuit_device.hip: prims_run_circuit_device, the product's k_circuit_* kernels).
// tests/test_prims_circuit.py calls both with plain arrays and compares every buffer with the Python oracle.
//
//   dims[CIRC_NDIMS] = N, nm, no, nv, k, f_l, f_m, rounds, nl, nn, NG, NH, form, W, label_len     (nl, nn: the proof's final scalars)
//   in[CIRC_NIN]     = label | fixed-base table of the 1 + NG + NH bases g | g_vec||g_vec_ | h_vec||h_vec_ (prims_bucket_fb_build)
//                      | commitments N x k x 64 | proofs N x proof_bytes | W_m | W_l | a_m | a_l (big-endian scalars, row-major)
//                      | part_lo | part_ll | part_lr | part_no (int32, -1 = None)
//   io[CIRC_NBUFS]   = the workspace buffers of CircuitWs in the kernels' own layout ([word][N] for the word arrays), handed in pre-filled
//                      (the caller's sentinel) and handed back as the stages left them; the last one, `plan`, CIRC_PLAN_WORDS int32: what
//                      plan_generic (plan_core.h) gave for the call -- c0_lanes, per_point, fb, tab_parts, fast, code
//   form: which of the three forms of C0's variable-base sum runs -- CIRC_VAR_POINTS: k_circuit_c0_var_pts on plan.c0_lanes lanes per
//         instance (refused where the plan has per_point clear: more than 64 points) | CIRC_VAR_TABLES: k_circuit_c0_tables, then
//         k_circuit_c0_var | CIRC_VAR_PROJECTIVE: k_circuit_c0_var with atab = nullptr (the projective-table Straus on w.straus).
// The launch choices are the plan's for a call of N instances on the default knobs (1,024 SIMDs), as circuit_verify_host_impl takes
// them: the fixed-base kernel from plan.fb, the lanes from plan.c0_lanes, the C0 points' tables behind 2 rounds tab_parts round-point tables.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../bp_pp_amd/csrc/circuit_core.h"
#include "../../bp_pp_amd/csrc/plan_core.h"

#define CIRC_NDIMS 15
#define CIRC_NIN 12
#define CIRC_NBUFS 14
#define CIRC_PLAN_WORDS 6
#define CIRC_VAR_POINTS 0
#define CIRC_VAR_TABLES 1
#define CIRC_VAR_PROJECTIVE 2
#define CIRC_MAX_N 4096

namespace circp {

enum In { I_LABEL, I_TABLE, I_COM, I_PROOFS, I_WM, I_WL, I_AM, I_AL, I_LO, I_LL, I_LR, I_NO };
enum Buf { B_STATUS, B_TSTATE, B_LAMV, B_MUV, B_COEF, B_SC0, B_PTS, B_ACC, B_PFIX, B_COMMIT, B_C, B_RHO, B_MU, B_PLAN };
static_assert(I_NO + 1 == CIRC_NIN && B_PLAN + 1 == CIRC_NBUFS, "buffer counts");

struct Shape {
    size_t N, nm, no, nv, k, nl_c, nw, rounds, nl, nn, NG, NH, W, label_len, proof_bytes;
    int f_l, f_m, form;
    bppp_host::GenericPlan plan;
    int atab_first;
};
// the bounds of bppp_circuit_create / circuit_verify_check (bppp_generic.hip) and of this launcher: every index the kernels form stays
// inside a buffer (the lane-per-point form writes table p at entries 16 p .. 16 p + 15 for p < 4 + k <= c0_lanes <= 64)
inline bool shape(Shape& s, const int64_t* d) {
    for (int i = 0; i < CIRC_NDIMS; i++)
        if (d[i] < 0 || d[i] > (1 << 20)) return false;
    s.N = (size_t)d[0]; s.nm = (size_t)d[1]; s.no = (size_t)d[2]; s.nv = (size_t)d[3]; s.k = (size_t)d[4]; s.f_l = (int)d[5]; s.f_m = (int)d[6];
    s.rounds = (size_t)d[7]; s.nl = (size_t)d[8]; s.nn = (size_t)d[9]; s.NG = (size_t)d[10]; s.NH = (size_t)d[11]; s.form = (int)d[12];
    s.W = (size_t)d[13]; s.label_len = (size_t)d[14];
    s.nl_c = s.nv * s.k; s.nw = 2 * s.nm + s.no;
    s.proof_bytes = 64 * (4 + 2 * s.rounds) + 32 * (s.nl + s.nn);
    if (s.N < 1 || s.N > CIRC_MAX_N || s.nm < 1 || s.nm > 64 || s.no > 64 || s.nv < 1 || s.nv > 64 || s.k < 1 || s.k > 124 || s.f_l > 1 || s.f_m > 1 ||
        s.nm > s.NG || s.nv + 9 > s.NH || s.NG > 64 || s.NH > 128 || s.rounds > 12 || s.nl > 4096 || s.nn > 4096 || s.W != 4 || s.label_len < 1 ||
        s.label_len > 255 || s.form > CIRC_VAR_PROJECTIVE)
        return false;
    const bppp_host::GenericKnobs knobs;
    s.plan = bppp_host::plan_generic(bppp_host::GENERIC_FORM_CIRCUIT, s.N, s.rounds, knobs, s.N, 1, 4 + s.k);
    if (s.form == CIRC_VAR_POINTS && (!s.plan.per_point || s.plan.c0_lanes > 64 || (size_t)s.plan.c0_lanes < 4 + s.k)) return false;
    if (s.form != CIRC_VAR_PROJECTIVE && !s.plan.fast) return false;
    s.atab_first = (int)(2 * s.rounds * 16 * (size_t)s.plan.tab_parts);      // wnla_atab_first (bppp_generic.hip)
    return true;
}
inline void sizes(const Shape& s, size_t in_bytes[CIRC_NIN], size_t io_bytes[CIRC_NBUFS]) {
    const size_t N = s.N;
    in_bytes[I_LABEL] = s.label_len; in_bytes[I_TABLE] = (1 + s.NG + s.NH) * bppp::fb_per_base((int)s.W) * sizeof(bppp::apt_packed);
    in_bytes[I_COM] = N * s.k * 64; in_bytes[I_PROOFS] = N * s.proof_bytes;
    in_bytes[I_WM] = s.nm * s.nw * 32; in_bytes[I_WL] = s.nl_c * s.nw * 32; in_bytes[I_AM] = s.nm * 32; in_bytes[I_AL] = s.nl_c * 32;
    in_bytes[I_LO] = in_bytes[I_LL] = in_bytes[I_LR] = s.nv * 4; in_bytes[I_NO] = s.nm * 4;
    io_bytes[B_STATUS] = N * 4; io_bytes[B_TSTATE] = 52 * N * 4; io_bytes[B_LAMV] = s.nl_c * 8 * N * 4; io_bytes[B_MUV] = s.nm * 8 * N * 4;
    io_bytes[B_COEF] = (3 * s.nm + 3 * s.nv) * 8 * N * 4; io_bytes[B_SC0] = (s.nm + 5 + s.k) * 8 * N * 4; io_bytes[B_PTS] = (4 + s.k) * 16 * N * 4;
    io_bytes[B_ACC] = 30 * N * 4; io_bytes[B_PFIX] = 30 * N * 4; io_bytes[B_COMMIT] = N * 64; io_bytes[B_C] = N * s.NH * 32; io_bytes[B_RHO] = N * 32;
    io_bytes[B_MU] = N * 32; io_bytes[B_PLAN] = CIRC_PLAN_WORDS * 4;
}
// scratch the stages keep to themselves, sized as wnla_fast_bytes sizes it (bppp_generic.hip): the window tables of the round points (not
// built here) with those of the 4 + k points behind them, entry-major; the running products of their build; the projective tables
inline size_t table_points(const Shape& s) { return 2 * s.rounds * (size_t)s.plan.tab_parts + 4 + s.k; }
inline size_t atab_entries(const Shape& s) { return table_points(s) * 16 * s.N; }
inline size_t tscr_words(const Shape& s) { return (size_t)BPPP_TSCR_PER_POINT * table_points(s) * 10 * s.N; }
inline size_t straus_slots(const Shape& s) { return s.N * 5 * BPPP_STRAUS_ENTRIES; }

// the circuit description on the host, as bppp_circuit_create builds it: circuit_host_build, the arrays never empty
inline bool host_data(bppp::CircuitHostData& hd, const Shape& s, const void* const* in) {
    const size_t dims[6] = {s.nm, s.no, s.k, s.nl_c, s.nv, s.nw};
    if (!bppp::circuit_host_build(hd, dims, (const uint8_t*)in[I_WM], (const uint8_t*)in[I_WL], (const uint8_t*)in[I_AM], (const uint8_t*)in[I_AL],
                                  (const int32_t*)in[I_LO], (const int32_t*)in[I_LL], (const int32_t*)in[I_LR], (const int32_t*)in[I_NO]))
        return false;
    hd.rl.push_back(0); hd.rm.push_back(0); hd.vl.resize(hd.vl.size() + 8); hd.vm.resize(hd.vm.size() + 8);
    return true;
}
// the nine arrays of CircuitDev in the order circuit_dev takes their addresses
inline void host_arrays(const bppp::CircuitHostData& hd, const void* ptr[9], size_t bytes[9]) {
    const void* p[9] = {hd.cpl.data(), hd.rl.data(), hd.vl.data(), hd.cpm.data(), hd.rm.data(), hd.vm.data(), hd.colmap.data(), hd.al.data(), hd.am.data()};
    const size_t b[9] = {hd.cpl.size() * 4, hd.rl.size() * 4, hd.vl.size() * 4, hd.cpm.size() * 4, hd.rm.size() * 4, hd.vm.size() * 4,
                         hd.colmap.size() * 4, hd.al.size() * 4, hd.am.size() * 4};
    for (int i = 0; i < 9; i++) { ptr[i] = p[i]; bytes[i] = b[i]; }
}
// the workspace as circuit_verify_host_impl fills it (bppp_generic.hip), over the caller's buffers; arr: the nine arrays where the
// stages read them (device copies, or the host's own)
inline bppp::CircuitWs workspace(const Shape& s, const uint8_t* label, const void* table, const void* com, const void* proofs, const void* const arr[9],
                                 void* const* io, bppp::apt_packed* atab, bppp::u32* tscr, bppp::pt_slot* straus) {
    using bppp::u32;
    bppp::CircuitWs r;
    memset(&r, 0, sizeof r);
    bppp::CircuitDev& cd = r.cd;
    cd.nm = (int)s.nm; cd.no = (int)s.no; cd.k = (int)s.k; cd.nl = (int)s.nl_c; cd.nv = (int)s.nv; cd.nw = (int)s.nw; cd.f_l = s.f_l; cd.f_m = s.f_m;
    cd.colptr_l = (const int*)arr[0]; cd.rows_l = (const int*)arr[1]; cd.vals_l = (const u32*)arr[2];
    cd.colptr_m = (const int*)arr[3]; cd.rows_m = (const int*)arr[4]; cd.vals_m = (const u32*)arr[5];
    cd.colmap = (const int*)arr[6]; cd.a_l = (const u32*)arr[7]; cd.a_m = (const u32*)arr[8];
    r.N = s.N; r.rounds = (int)s.rounds; r.NG = (int)s.NG; r.NH = (int)s.NH; r.proof_bytes = s.proof_bytes;
    r.commitments = (const uint8_t*)com; r.proofs = (const uint8_t*)proofs;
    r.status = (int32_t*)io[B_STATUS]; r.tstate = (u32*)io[B_TSTATE]; r.lamv = (u32*)io[B_LAMV]; r.muv = (u32*)io[B_MUV]; r.coef = (u32*)io[B_COEF];
    r.sc0 = (u32*)io[B_SC0]; r.pts = (u32*)io[B_PTS]; r.acc = (u32*)io[B_ACC]; r.pfix = (u32*)io[B_PFIX];
    r.wn_commit = (uint8_t*)io[B_COMMIT]; r.wn_c = (uint8_t*)io[B_C]; r.wn_rho = (uint8_t*)io[B_RHO]; r.wn_mu = (uint8_t*)io[B_MU];
    r.straus = straus;
    r.atab = s.form == CIRC_VAR_PROJECTIVE ? nullptr : atab; r.tscr = tscr; r.atab_first = s.atab_first;
    r.fb.table = (const bppp::apt_packed*)table; r.fb.W = (int)s.W; r.fb.N = s.N;
    bppp::t_new(r.base, label, (u32)s.label_len);
    return r;
}
inline void plan_words(const Shape& s, int32_t out[CIRC_PLAN_WORDS]) {
    out[0] = s.plan.c0_lanes; out[1] = s.plan.per_point ? 1 : 0; out[2] = s.plan.fb; out[3] = s.plan.tab_parts; out[4] = s.plan.fast ? 1 : 0;
    out[5] = (int32_t)s.plan.code();
}

}  // namespace circp
