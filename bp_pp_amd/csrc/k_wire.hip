// Wire form of the generic proofs: SEC1 expand / compress over a WireMap (wire_core.h), any layout.
// Part of libbppp_hip.so; the lane functions live in wire_core.h, declarations in kernels.h.
#include "kernels.h"

using namespace bppp;

// one lane per point (then per scalar word) over the flat batch: m.first[m.nseg] lanes
__global__ __launch_bounds__(256) void k_wire_expand(WireMap m) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g < m.first[m.nseg]) wire_expand_lane(m, g);
}
__global__ __launch_bounds__(256) void k_wire_compress(WireMap m) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g < m.first[m.nseg]) wire_compress_lane(m, g);
}
