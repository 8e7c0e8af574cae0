// TEST-ONLY gfx950 launcher of the product's own aggregate kernels: the verifier's phase 1 and C0 stage (k_agg.hip) and the prover's
// witness, r1 and r2 stages (k_aggprove.hip).  Both translation units are included as they are, so this unit of libbppp_prims_hip.so
// holds the code the product runs, compiled with the product's flags (tests/prims/build.py), launched with the product's grids, and
// every buffer the stages write goes back to the caller (agg_prims.h has the arguments).
// A unit of its own: the kernel units say `using namespace bppp`, which must not meet prims_core.h's namespace prims.
#include "../../bp_pp_amd/csrc/k_agg.hip"
#include "../../bp_pp_amd/csrc/k_aggprove.hip"

#include "agg_prims.h"

#define PRIMS_API extern "C" __attribute__((visibility("default")))

// the grids of bppp_generic.hip, where they are static functions of these names: blocks_of, fb_blocks_of, fb64_blocks_of, fb1_blocks_of
static unsigned blocks_of(size_t n) { return (unsigned)((n + BPPP_BLOCK - 1) / BPPP_BLOCK); }
static unsigned fb_blocks_of(size_t n) { return (unsigned)((n * BPPP_FB_LANES + BPPP_FB_BLOCK - 1) / BPPP_FB_BLOCK); }
static unsigned fb64_blocks_of(size_t n) { return (unsigned)((n * 64 + BPPP_FB_BLOCK - 1) / BPPP_FB_BLOCK); }
static unsigned fb1_blocks_of(size_t n) { return (unsigned)((n + BPPP_FB_BLOCK - 1) / BPPP_FB_BLOCK); }

__global__ __launch_bounds__(BPPP_BLOCK) void k_aggp_fallback_mask(AggWs w, uint8_t* fell) {
    size_t t = (size_t)blockIdx.x * BPPP_BLOCK + threadIdx.x;
    if (t < w.N) fell[t] = aggp::fallback_mask(w, t);
}

namespace {
struct DevBuf {      // one device allocation, freed when the launcher returns
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t up(const void* src, size_t bytes) {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
        if (e == hipSuccess && src && bytes) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
        return e;
    }
    hipError_t down(void* dst, size_t bytes) const { return bytes ? hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
};
}  // namespace

// The launch sequence of agg_verify_device_impl (bppp_generic.hip; its uniform form, without the caller's transcripts) on the null stream, the form word in place of the plan.
// Returns the first HIP error (hipErrorInvalidValue for arguments out of range: nothing is launched then).
PRIMS_API int prims_run_agg_verify_device(const int64_t* dims, const void* const* in, void* const* io) {
    aggp::VerifyShape s;
    if (!aggp::verify_shape(s, dims)) return (int)hipErrorInvalidValue;
    size_t in_bytes[4], io_bytes[AGGV_NBUFS];
    aggp::verify_sizes(s, in_bytes, io_bytes);
    DevBuf din[4], dio[AGGV_NBUFS], datab, dtscr, dstraus;
    hipError_t e = hipSuccess;
    for (int i = 1; i < 4 && e == hipSuccess; i++) e = din[i].up(in[i], in_bytes[i]);
    void* dptr[AGGV_NBUFS];
    for (int i = 0; i < AGGV_NBUFS && e == hipSuccess; i++) { e = dio[i].up(io[i], io_bytes[i]); dptr[i] = dio[i].p; }
    if (e == hipSuccess) e = datab.up(nullptr, aggp::verify_atab_entries(s) * sizeof(apt_packed));
    if (e == hipSuccess) e = dtscr.up(nullptr, aggp::verify_tscr_words(s) * sizeof(u32));
    if (e == hipSuccess) e = dstraus.up(nullptr, aggp::verify_straus_slots(s) * sizeof(pt_slot));
    if (e != hipSuccess) return (int)e;
    const AggWs r = aggp::verify_ws(s, (const uint8_t*)in[0], din[1].p, din[2].p, din[3].p, dptr, (apt_packed*)datab.p, (u32*)dtscr.p,
                                    (pt_slot*)dstraus.p);
    const size_t n = s.N;
    const unsigned blocks = blocks_of(n);
    const int G = s.G;
    if (G > 1) k_agg_phase1_grp<<<(unsigned)(((size_t)G * n + BPPP_BLOCK - 1) / BPPP_BLOCK), BPPP_BLOCK, 0, 0>>>(r, G);
    else k_agg_phase1<<<blocks, BPPP_BLOCK, 0, 0>>>(r);
    e = hipGetLastError();
    if (e == hipSuccess) {
        if (s.fb == AGGV_FB_L1) k_agg_c0_fixed_l1<<<fb1_blocks_of(n), BPPP_FB_BLOCK, 0, 0>>>(r);
        else if (s.fb == AGGV_FB_L64) k_agg_c0_fixed_l64<<<fb64_blocks_of(n), BPPP_FB_BLOCK, 0, 0>>>(r);
        else k_agg_c0_fixed<<<fb_blocks_of(n), BPPP_FB_BLOCK, 0, 0>>>(r);
        e = hipGetLastError();
    }
    if (e == hipSuccess && r.atab) { k_agg_c0_tables<<<blocks, BPPP_BLOCK, 0, 0>>>(r); e = hipGetLastError(); }
    if (e == hipSuccess) { k_agg_c0_var<<<blocks, BPPP_BLOCK, 0, 0>>>(r); e = hipGetLastError(); }
    if (e == hipSuccess) { k_agg_c0_finish<<<blocks, BPPP_BLOCK, 0, 0>>>(r); e = hipGetLastError(); }
    // (behind the product's sequence: the tables and scalars it reads are still what k_agg_c0_var read)
    if (e == hipSuccess) { k_aggp_fallback_mask<<<blocks, BPPP_BLOCK, 0, 0>>>(r, (uint8_t*)dptr[aggp::V_FELL]); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (int i = 0; i < AGGV_NBUFS && e == hipSuccess; i++) e = dio[i].down(io[i], io_bytes[i]);
    return (int)e;
}

// k_aprove_witness, k_aprove_stage_r1, k_aprove_msm, k_aprove_stage_r2 with agg_prove_part's grids (bppp_generic.hip: blocks_of(n)
// blocks of BPPP_BLOCK; the msm fb_blocks_of(n k) blocks of BPPP_FB_BLOCK).  Returns the first HIP error (hipErrorInvalidValue for arguments out of range).
PRIMS_API int prims_run_agg_prove_device(const int64_t* dims, const void* const* in, void* const* io) {
    aggp::ProveShape s;
    if (!aggp::prove_shape(s, dims)) return (int)hipErrorInvalidValue;
    size_t io_bytes[AGGP_NBUFS];
    aggp::prove_sizes(s, io_bytes);
    if ((s.stages & AGGP_MSM) && !in[1]) return (int)hipErrorInvalidValue;
    DevBuf dio[AGGP_NBUFS], dtable;
    void* dptr[AGGP_NBUFS];
    hipError_t e = (s.stages & AGGP_MSM) ? dtable.up(in[1], aggp::prove_table_bytes(s)) : hipSuccess;
    for (int i = 0; i < AGGP_NBUFS && e == hipSuccess; i++) { e = dio[i].up(io[i], io_bytes[i]); dptr[i] = dio[i].p; }
    if (e != hipSuccess) return (int)e;
    const AggProveWs a = aggp::prove_ws(s, (const uint8_t*)in[0], dtable.p, dptr);
    const unsigned blocks = blocks_of(s.N);
    if (s.stages & AGGP_WITNESS) { k_aprove_witness<<<blocks, BPPP_BLOCK, 0, 0>>>(a); e = hipGetLastError(); }
    if (e == hipSuccess && (s.stages & AGGP_R1)) { k_aprove_stage_r1<<<blocks, BPPP_BLOCK, 0, 0>>>(a); e = hipGetLastError(); }
    if (e == hipSuccess && (s.stages & AGGP_MSM)) { k_aprove_msm<<<fb_blocks_of(s.N * s.k), BPPP_FB_BLOCK, 0, 0>>>(a); e = hipGetLastError(); }
    if (e == hipSuccess && (s.stages & AGGP_R2)) { k_aprove_stage_r2<<<blocks, BPPP_BLOCK, 0, 0>>>(a); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (int i = 0; i < AGGP_NBUFS && e == hipSuccess; i++) e = dio[i].down(io[i], io_bytes[i]);
    return (int)e;
}
