// TEST-ONLY gfx950 build of the primitive dispatcher (prims_core.h): one record per lane, compiled with the product's own flags
// (bp_pp_amd/_build.py BASE_FLAGS) by tests/prims/build.py into libbppp_prims_hip.so.
#include <hip/hip_runtime.h>

#include "prims_core.h"

#define PRIMS_API extern "C" __attribute__((visibility("default")))

__global__ __launch_bounds__(64) void k_prims(const uint32_t* in, uint32_t* out, size_t n, const uint8_t* bytes, size_t nbytes) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint32_t* rin = in + r * PRIM_IN_WORDS;
    prims::prim_eval(rin[0], rin, out + r * PRIM_OUT_WORDS, bytes, nbytes);
}

PRIMS_API int prims_record_words(int which) { return which == 0 ? PRIM_IN_WORDS : PRIM_OUT_WORDS; }
// Copies n records (and the byte side input) to the device, evaluates them, copies the results back.  Returns the first HIP error.
PRIMS_API int prims_run_device(const uint32_t* in, uint32_t* out, size_t n, const uint8_t* bytes, size_t nbytes) {
    if (n == 0) return 0;
    uint32_t *din = nullptr, *dout = nullptr;
    uint8_t* dbytes = nullptr;
    const size_t in_sz = n * PRIM_IN_WORDS * sizeof(uint32_t), out_sz = n * PRIM_OUT_WORDS * sizeof(uint32_t);
    const size_t b_sz = nbytes ? nbytes : 1;
    hipError_t e = hipMalloc((void**)&din, in_sz);
    if (e == hipSuccess) e = hipMalloc((void**)&dout, out_sz);
    if (e == hipSuccess) e = hipMalloc((void**)&dbytes, b_sz);
    if (e == hipSuccess) e = hipMemcpy(din, in, in_sz, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0, out_sz);
    if (e == hipSuccess && nbytes) e = hipMemcpy(dbytes, bytes, nbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const unsigned blocks = (unsigned)((n + 63) / 64);
        hipLaunchKernelGGL(k_prims, dim3(blocks), dim3(64), 0, 0, din, dout, n, dbytes, nbytes);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, out_sz, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    if (dbytes) (void)hipFree(dbytes);
    return (int)e;
}
