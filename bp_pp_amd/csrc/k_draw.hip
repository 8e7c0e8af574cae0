// The seeded provers' draws: ChaCha20 blocks reduced mod n (draw_core.h), one (instance, draw) pair per lane.
// Part of libbppp_hip.so; the lane code lives in draw_core.h, the declaration in kernels.h.
#include "kernels.h"

using namespace bppp;

// lane g = i k + j writes draw j of instance i (stream stream_base + i, block j) as 32 big-endian bytes at out + 32 g: the `rnd`
// layout (n x k x 32), so consecutive lanes store consecutive scalars, two 16-byte stores each.  The key and the stream base are
// kernel arguments; the only branch is the grid tail.
__global__ __launch_bounds__(256) void k_draw_scalars(DrawKey key, u64 stream_base, u64 k, u64 total, uint8_t* out) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const u64 i = g / k, j = g - i * k;
    u32 w[8];
    draw_scalar_words(w, key.w, stream_base + i, j);
    uint4* o = reinterpret_cast<uint4*>(out + g * 32);
    o[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
