// Wire form of the aggregate's mixed-value-count call: SEC1 expansion of slots laid out by k_max, every instance on its own k_t
// (wire_mixed_core.h).  Part of libbppp_hip.so; a translation unit of its own, so that the code objects of k_wire.hip stay what they were.
#include "kernels.h"

using namespace bppp;

// one lane per point slot of the k_max layout, then per scalar word: wire_mixed_lanes(m) lanes; the lanes behind k_t idle
__global__ __launch_bounds__(256) void k_wire_expand_mixed(WireMixed m) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g < wire_mixed_lanes(m)) wire_mixed_expand_lane(m, g);
}
