// aggregated reciprocal range proof PROVER for mixed value counts (agg_prove_mixed_core.h): the witness, stages r1 / r2, the circuit
// prover's stages A, B, C on every instance's own k_t, and the assembly.  The fixed-base sums, stage D and the WNLA prover are the
// uniform kernels (k_gprove.hip, k_aggprove.hip) over the k_max shape.  Part of libbppp_hip.so; a translation unit of its own, so that
// the code objects of the uniform provers' kernels stay what they were.
// Per-lane trip counts differ inside a wavefront here: a wavefront takes the time of its largest k_t; r1's head and stage B it runs
// once per value count present in it.
#include "kernels.h"

using namespace bppp;

__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_mixed_witness(AggProveMixedWs m) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < m.a.N) agg_prove_mixed_witness(m, t);
}
// r1's transcript takes k_t points before its challenge, and the transcript code holds the sponge position in a scalar register: the
// head runs once per value count present in the wavefront (lanes of one count share every position), as k_agg_mixed_phase1's does
__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_mixed_stage_r1(AggProveMixedWs m) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t >= m.a.N) return;
    bool bad_k, ok = true;
    const int k = agg_prove_mixed_k(m.ks, m.a.k, t, bad_k);
    int32_t status = 0;
    sc e;
    for_each_position_group((u32)k, [&]() { agg_prove_mixed_r1_head(m, t, k, status, ok, e); });
    agg_prove_mixed_r1_rest(m, t, k, bad_k, status, ok, e);
}
__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_mixed_stage_r2(AggProveMixedWs m) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < m.a.N) agg_prove_mixed_stage_r2(m, t);
}
__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_mixed_stage_a(CircuitProveMixedWs m) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < m.p.N) agg_prove_mixed_stage_a(m, t);
}
// Stage B takes k_t "commitment_v" points before circuit_rho, so it too runs once per value count.  It is the chain's largest kernel
// (every register, and scratch beside them), and a loop over the wavefront's counts around it took 3,856 bytes of scratch per lane
// where the uniform stage takes 2,240 -- scratch the runtime sizes for a full device and keeps per hardware queue.  So the HOST walks the
// counts: one launch per k of 1 .. k_max, in which the lanes of that count run and the others leave; k is a kernel argument, the
// trip counts are scalar as in the uniform kernel, and a wavefront still pays stage B once per count present in it.
__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_mixed_stage_b(CircuitProveMixedWs m, int k) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t >= m.p.N || agg_prove_mixed_ck(m, t) != k) return;
    agg_prove_mixed_stage_b(m, t, k);
}
__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_mixed_collect(CircuitProveMixedWs m) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < m.p.N) agg_prove_mixed_collect_again(m, t);
}
// every challenge squeezes from position 0: stage C starts at one position whatever k_t
__global__ __launch_bounds__(BPPP_BLOCK) void k_aprove_mixed_stage_c(CircuitProveMixedWs m) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < m.p.N) agg_prove_mixed_stage_c(m, t);
}
__global__ __launch_bounds__(256) void k_aprove_mixed_assemble(ProofAssembleMixedWs m) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, words = m.w.proof_bytes / 4;
    if (g < m.w.N * words) proof_assemble_mixed_word(m, g / words, (u32)(g % words));
}
