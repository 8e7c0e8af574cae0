// aggregated reciprocal range proof PROVER kernels (agg_prove_core.h): the witness of k values, stages r1 / r2 and the pole commitments'
// sum over N k rows, and the circuit prover's stage B with the closed-form collect.  Everything else of the chain is k_gprove.hip's
// (k_rprove_commit*, k_cprove_*, k_wprove_*, k_gprove_assemble).  Part of libbppp_hip.so; a translation unit of its own, so that the
// code objects of the other provers' kernels stay what they were.
#include "kernels.h"

using namespace bppp;

__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_witness(AggProveWs w) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < w.N) agg_prove_witness(w, t);
}
// On the CALLER'S transcripts (the _transcript entry points) stage r1 and stage B run as the _tx kernels, kernels of their own so that
// the label forms' code objects stay what they were: once per sponge position in the wavefront when the states are per-instance
// (kernels.h: for_each_position_group), one trip when the state is shared
template <typename Ws>
__device__ __forceinline__ u32 aprove_position_key(const Ws& w, size_t t) {
    return w.divergent_positions ? preloaded_position_key(w.tio.states, w.tio.n_states, t) : 0u;
}
__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_stage_r1(AggProveWs w) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < w.N) agg_prove_stage_r1(w, t);
}
__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_stage_r1_tx(AggProveWs w) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t >= w.N) return;
    for_each_position_group(aprove_position_key(w, t), [&]() { agg_prove_stage_r1<true>(w, t); });
}
// R_i = rb_i h_vec[0] + sum_d r_{i,d} h_vec[9 + d]: BPPP_FB_LANES lanes per row, N k rows
__global__ __launch_bounds__(BPPP_FB_BLOCK, BPPP_FB_MIN_WAVES) void k_aprove_msm(AggProveWs w) {
    size_t g = (size_t)blockIdx.x * BPPP_FB_BLOCK + threadIdx.x;
    size_t row = g / BPPP_FB_LANES;
    int lane = (int)(g % BPPP_FB_LANES);
    const size_t rows = w.N * (size_t)w.k;
    if (row >= rows) return;
    pt part;
    FbRanges rg;
    agg_prove_pole_ranges(rg, w);
    if (w.ct) fb_group_sum_ct<BPPP_FB_LANES>(part, w.fb_ct, row, lane, w.rsc, rg);
    else fb_group_sum(part, w.fb, row, lane, w.rsc, rg);
    if (lane == 0) ws_st_pt(w.rpb, rows, row, part);
}
__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_stage_r2(AggProveWs w) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < w.N) agg_prove_stage_r2(w, t);
}
// every instance starts from Transcript::new(label): one sponge position in the wavefront, no position groups
__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_stage_b(CircuitProveWs w) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < w.N) agg_prove_stage_b(w, t);
}
__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_stage_b_tx(CircuitProveWs w) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t >= w.N) return;
    for_each_position_group(aprove_position_key(w, t), [&]() { agg_prove_stage_b(w, t); });
}
__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_collect(CircuitProveWs w) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < w.N) agg_collect_again(w, t);
}
// the caller's `&mut Transcript` after a prove from integers (agg_prove_core.h: agg_prove_export)
__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_export_states(TranscriptIo io, strobe base, const u32* tstate, size_t N, const int32_t* status) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < N) agg_prove_export(io, base, tstate, N, status, t);
}
