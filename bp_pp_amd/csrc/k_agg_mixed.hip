// aggregated reciprocal range proofs of mixed value counts (agg_mixed_core.h): phase 1 and the variable-base half of C0 on every
// instance's own k_t.  The fixed-base half, the finish and the WNLA stage are the uniform kernels of k_agg.hip and k_generic.hip.
// Part of libbppp_hip.so; a translation unit of its own, so that the code objects of the uniform kernels stay what they were.
// Per-lane trip counts differ inside a wavefront here: behind phase 1's head a wavefront takes the time of its largest k_t.
#include "kernels.h"

using namespace bppp;

// The head's transcript sits at a sponge position that depends on k_t, and the transcript code holds the position in a scalar
// register: the head runs once per value count present in the wavefront (lanes of one count share every position), as the kernels
// on per-instance pre-loaded transcripts run once per position.  It starts and ends at one position whatever k_t
// (agg_mixed_core.h), so the rest of phase 1 and every kernel behind it run undivided.
__device__ __forceinline__ void agg_mixed_phase1_lanes(const AggMixedWs& m, size_t t, int q, int G) {
    AggHead h;
    bool bad;
    const int k = agg_mixed_k(m, t, bad);
    for_each_position_group((u32)k, [&]() { agg_mixed_phase1_head(m, t, k, bad, h); });
    agg_mixed_phase1_rest(m, t, k, h, q, G);
}
__global__ __launch_bounds__(BPPP_BLOCK) void k_agg_mixed_phase1(AggMixedWs m) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < m.w.N) agg_mixed_phase1_lanes(m, t, 0, 1);
}
// G = 2, 4 or 8 lanes per instance: the lanes of a group share their instance and so its k_t and its trip counts
__global__ __launch_bounds__(BPPP_BLOCK) void k_agg_mixed_phase1_grp(AggMixedWs m, int G) {
    const size_t g = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    const size_t t = g / (size_t)G;
    if (t >= m.w.N) return;                   // whole groups leave together (G divides the block)
    agg_mixed_phase1_lanes(m, t, (int)(g % (size_t)G), G);
}
__global__ __launch_bounds__(BPPP_BLOCK, BPPP_TABLES_MIN_WAVES) void k_agg_mixed_c0_tables(AggMixedWs m) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < m.w.N) agg_mixed_c0_tables(m, t);
}
__global__ __launch_bounds__(BPPP_BLOCK) void k_agg_mixed_c0_var(AggMixedWs m) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < m.w.N) agg_mixed_c0_var(m, t);
}
