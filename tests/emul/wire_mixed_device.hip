// TEST-ONLY device runner of the product's own k_wire_expand_mixed: bp_pp_amd/csrc/k_wire_mixed.hip included as it is, and one C
// function that launches the kernel over device pointers as agg_sec1_run does for a mixed call (tests/emul/build_wire_mixed.py builds it with
// hipcc for gfx950; tests/test_gpu_agg_mixed_wire_expand.py checks the bytes it leaves).
#include "../../bp_pp_amd/csrc/k_wire_mixed.hip"

extern "C" __attribute__((visibility("default"))) int wire_mixed_run_device(const void* d_com33, const void* d_proofs33, void* d_com64,
                                                                            void* d_proofs64, const void* d_ks, size_t n, int k_max,
                                                                            int rounds, int ns) {
    WireMixed m;
    m.com33 = (const uint8_t*)d_com33; m.proofs33 = (const uint8_t*)d_proofs33; m.com64 = (uint8_t*)d_com64;
    m.proofs64 = (uint8_t*)d_proofs64; m.ks = (const uint8_t*)d_ks;
    m.n = n; m.k_max = (u32)k_max; m.rounds = (u32)rounds; m.ns = (u32)ns;
    const u64 lanes = wire_mixed_lanes(m);
    if (lanes == 0) return 0;
    k_wire_expand_mixed<<<(unsigned)((lanes + 255) / 256), 256, 0, 0>>>(m);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return (int)e;
}
