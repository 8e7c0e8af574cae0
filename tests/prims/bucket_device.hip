// TEST-ONLY gfx950 launcher of the product's own bucket-stage kernels (k_bkt_prepare, k_bkt_accumulate, k_bkt_scalars, k_bkt_check):
// the kernels' translation unit is included as it is, so this unit of libbppp_prims_hip.so holds the code the product runs, compiled
// with the product's flags (tests/prims/build.py), and hands every intermediate value back (bucket_prims.h has the arguments).
// A unit of its own: k_verify_bucket.hip says `using namespace bppp`, which must not meet prims_core.h's namespace prims.
#include "../../bp_pp_amd/csrc/k_verify_bucket.hip"

#include "bucket_prims.h"

#define PRIMS_API extern "C" __attribute__((visibility("default")))

static_assert(sizeof(bppp::c4_packed) == 96 && sizeof(bppp::apt_packed) == 64, "the packed layouts the tests write");

PRIMS_API size_t prims_bucket_fb_entries(int nb, int W) { return bktp::fb_entries(nb, W); }
// built on the host by the product's fb_build_pass1 / fb_build_pass2, copied to the device by prims_run_bucket_device
PRIMS_API int prims_bucket_fb_build(const uint8_t* gens, int nb, int W, uint8_t* table_out) {
    if (nb < 1 || nb > BKT_MAX_NB || W != 4) return -1;
    return bktp::fb_build(gens, nb, W, table_out);
}
PRIMS_API void prims_bucket_geometry(uint32_t M, int nb, uint64_t out[2]) { out[0] = bkt_lds_bytes(M); out[1] = bkt_scalar_groups(nb); }

namespace {
struct DevBuf {      // one device allocation, freed when the launcher returns
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t up(const void* src, size_t bytes) {
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess && src) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
        return e;
    }
    hipError_t fill(int byte, size_t bytes) {
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) e = hipMemset(p, byte, bytes);
        return e;
    }
    hipError_t down(void* dst, size_t bytes) const { return hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost); }
};
}  // namespace

// Launches the four kernels with launch_bucket_stage's geometry (host.h) on the null stream.  Returns the first HIP error
// (hipErrorInvalidValue for arguments out of range: nothing is launched then).
PRIMS_API int prims_run_bucket_device(size_t N, uint32_t M, int nb, const uint64_t* seed, const int32_t* status, const uint32_t* acc,
                                      const uint32_t* fsc, const uint8_t* table, int W, int given, uint64_t* wab, uint32_t* c4, uint32_t* lhs,
                                      uint32_t* asc, uint8_t* sflag, uint8_t* accept) {
    if (!bktp::args_ok(N, M, nb, W)) return (int)hipErrorInvalidValue;
    const size_t ns = bktp::nsuper_of(N, M);
    const size_t wab_sz = N * 16, c4_sz = N * sizeof(c4_packed), lhs_sz = ns * 30 * 4, asc_sz = ns * (size_t)nb * 32;
    DevBuf dstatus, dacc, dfsc, dtable, dwab, dc4, dlhs, dasc, dsflag, daccept;
    hipError_t e = dstatus.up(status, N * sizeof(int32_t));
    if (e == hipSuccess) e = dacc.up(acc, N * 30 * 4);
    if (e == hipSuccess) e = dfsc.up(fsc, N * (size_t)nb * 32);
    if (e == hipSuccess) e = dtable.up(table, bktp::fb_entries(nb, W) * sizeof(apt_packed));
    if (e == hipSuccess) e = given ? dwab.up(wab, wab_sz) : dwab.fill(0, wab_sz);
    if (e == hipSuccess) e = given ? dc4.up(c4, c4_sz) : dc4.fill(0, c4_sz);
    if (e == hipSuccess) e = dlhs.fill(0, lhs_sz);
    if (e == hipSuccess) e = dasc.fill(0, asc_sz);
    if (e == hipSuccess) e = dsflag.fill(BKT_SENTINEL, ns);
    if (e == hipSuccess) e = daccept.fill(BKT_SENTINEL, N);
    if (e != hipSuccess) return (int)e;
    const BucketWs bw = bktp::workspace(N, M, nb, seed, (const int32_t*)dstatus.p, (const u32*)dacc.p, (const u32*)dfsc.p, (const uint8_t*)dtable.p, W,
                                        (uint64_t*)dwab.p, (uint32_t*)dc4.p, (uint32_t*)dlhs.p, (uint32_t*)dasc.p, (uint8_t*)dsflag.p,
                                        (uint8_t*)daccept.p);
    const size_t lds_bytes = bkt_lds_bytes(M);
    e = hipFuncSetAttribute((const void*)k_bkt_accumulate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    const unsigned blocks = (unsigned)((N + BPPP_BLOCK - 1) / BPPP_BLOCK);
    const dim3 sgrid((unsigned)ns, bkt_scalar_groups(nb));
    if (e == hipSuccess && !given) { k_bkt_prepare<<<blocks, BPPP_BLOCK, 0, 0>>>(bw); e = hipGetLastError(); }
    if (e == hipSuccess) { k_bkt_accumulate<<<(unsigned)ns, 256, lds_bytes, 0>>>(bw); e = hipGetLastError(); }
    if (e == hipSuccess) { k_bkt_scalars<<<sgrid, 256, 0, 0>>>(bw); e = hipGetLastError(); }
    if (e == hipSuccess) { k_bkt_check<<<(unsigned)ns, 64, 0, 0>>>(bw); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = dwab.down(wab, wab_sz);
    if (e == hipSuccess) e = dc4.down(c4, c4_sz);
    if (e == hipSuccess) e = dlhs.down(lhs, lhs_sz);
    if (e == hipSuccess) e = dasc.down(asc, asc_sz);
    if (e == hipSuccess) e = dsflag.down(sflag, ns);
    if (e == hipSuccess) e = daccept.down(accept, N);
    return (int)e;
}
