// aggregated reciprocal range proof verifier kernels (agg_core.h): phase 1 and the C0 stage; the WNLA stage behind them is k_generic.hip's.
// Part of libbppp_hip.so; a translation unit of its own, so that the code objects of the other verifiers' kernels stay what they were.
#include "kernels.h"

using namespace bppp;

__global__ __launch_bounds__(BPPP_BLOCK) void k_agg_phase1(AggWs w) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < w.N) agg_phase1(w, t);
}
// G = 2, 4 or 8 lanes per instance (agg_core.h: agg_phase1): calls whose one-lane kernels leave wavefront slots free
__global__ __launch_bounds__(BPPP_BLOCK) void k_agg_phase1_grp(AggWs w, int G) {
    const size_t g = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    const size_t t = g / (size_t)G;
    if (t >= w.N) return;                     // whole groups leave together (G divides the block)
    agg_phase1(w, t, (int)(g % (size_t)G), G);
}
// The same two on the CALLER'S transcripts (w.tio.states set: the _transcript entry points), kernels of their own so that the label
// forms' code objects above stay what they were.  Per-instance states may sit at different sponge positions: the body runs once per
// position present in the wavefront (kernels.h: for_each_position_group), one trip when the state is shared.
__global__ __launch_bounds__(BPPP_BLOCK) void k_agg_phase1_tx(AggWs w) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t >= w.N) return;
    const u32 key = preloaded_position_key(w.tio.states, w.tio.n_states, t);
    for_each_position_group(key, [&]() { agg_phase1<true>(w, t); });
}
__global__ __launch_bounds__(BPPP_BLOCK) void k_agg_phase1_grp_tx(AggWs w, int G) {
    const size_t g = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    const size_t t = g / (size_t)G;
    if (t >= w.N) return;                     // whole groups leave together (G divides the block)
    const int q = (int)(g % (size_t)G);
    const u32 key = preloaded_position_key(w.tio.states, w.tio.n_states, t);      // (the lanes of a group share their instance's key)
    for_each_position_group(key, [&]() { agg_phase1<true>(w, t, q, G); });
}
template <int NL>
__device__ __forceinline__ void agg_c0_fixed_lanes(const AggWs& w) {
    size_t g = (size_t)blockIdx.x * BPPP_FB_BLOCK + threadIdx.x;
    size_t t = g / NL;
    int lane = (int)(g % NL);
    if (t >= w.N) return;
    pt part;
    FbRanges rg;
    agg_c0_fixed_ranges(rg, w);
    fb_group_sum<NL>(part, w.fb, t, lane, w.sc0, rg);
    if (lane == 0) agg_c0_fixed_store(w, t, part);
}
__global__ __launch_bounds__(BPPP_FB_BLOCK, BPPP_FB_MIN_WAVES) void k_agg_c0_fixed(AggWs w) { agg_c0_fixed_lanes<BPPP_FB_LANES>(w); }
__global__ __launch_bounds__(BPPP_FB_BLOCK, BPPP_FB_MIN_WAVES) void k_agg_c0_fixed_l1(AggWs w) { agg_c0_fixed_lanes<1>(w); }
__global__ __launch_bounds__(BPPP_FB_BLOCK, BPPP_FB_MIN_WAVES) void k_agg_c0_fixed_l64(AggWs w) { agg_c0_fixed_lanes<64>(w); }
__global__ __launch_bounds__(BPPP_BLOCK, BPPP_TABLES_MIN_WAVES) void k_agg_c0_tables(AggWs w) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < w.N) agg_c0_tables(w, t);
}
__global__ __launch_bounds__(BPPP_BLOCK) void k_agg_c0_var(AggWs w) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < w.N) agg_c0_var(w, t);
}
__global__ __launch_bounds__(BPPP_BLOCK) void k_agg_c0_finish(AggWs w) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < w.N) agg_c0_finish(w, t);
}
