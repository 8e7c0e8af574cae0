// TEST-ONLY gfx950 launcher of the product's own circuit-stage kernels: phase 1 and the C0 stage of the generic ArithmeticCircuit verifier
// (k_generic.hip, circuit_core.h).  The translation unit is included as it is, so this unit of libbppp_prims_hip.so holds the code the
// product runs, compiled with the product's flags (tests/prims/build.py), launched with the product's grids on the plan's choices, and
// every buffer the stages write goes back to the caller (circuit_prims.h has the arguments).
// A unit of its own: the kernel unit says `using namespace bppp`, which must not meet prims_core.h's namespace prims.
#include "../../bp_pp_amd/csrc/k_generic.hip"

#include "circuit_prims.h"

#define PRIMS_API extern "C" __attribute__((visibility("default")))

// the grids of bppp_generic.hip, where they are static functions of these names: blocks_of, fb_blocks_of, fb64_blocks_of
static unsigned blocks_of(size_t n) { return (unsigned)((n + BPPP_BLOCK - 1) / BPPP_BLOCK); }
static unsigned fb_blocks_of(size_t n) { return (unsigned)((n * BPPP_FB_LANES + BPPP_FB_BLOCK - 1) / BPPP_FB_BLOCK); }
static unsigned fb64_blocks_of(size_t n) { return (unsigned)((n * 64 + BPPP_FB_BLOCK - 1) / BPPP_FB_BLOCK); }

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

// The launch sequence of circuit_verify_host_impl (bppp_generic.hip) up to k_circuit_c0_finish, on the null stream, the plan taken from
// plan_generic for a call of N instances and the form word choosing among the three forms of the variable-base sum.
// Returns the first HIP error (hipErrorInvalidValue for arguments out of range: nothing is launched then).
PRIMS_API int prims_run_circuit_device(const int64_t* dims, const void* const* in, void* const* io) {
    circp::Shape s;
    if (!circp::shape(s, dims)) return (int)hipErrorInvalidValue;
    CircuitHostData hd;
    if (!circp::host_data(hd, s, in)) return (int)hipErrorInvalidValue;
    size_t in_bytes[CIRC_NIN], io_bytes[CIRC_NBUFS], arr_bytes[9];
    circp::sizes(s, in_bytes, io_bytes);
    const void* harr[9];
    circp::host_arrays(hd, harr, arr_bytes);
    DevBuf dtable, dcom, dproofs, darr[9], dio[CIRC_NBUFS], datab, dtscr, dstraus;
    hipError_t e = dtable.up(in[circp::I_TABLE], in_bytes[circp::I_TABLE]);
    if (e == hipSuccess) e = dcom.up(in[circp::I_COM], in_bytes[circp::I_COM]);
    if (e == hipSuccess) e = dproofs.up(in[circp::I_PROOFS], in_bytes[circp::I_PROOFS]);
    const void* arr[9];
    for (int i = 0; i < 9 && e == hipSuccess; i++) { e = darr[i].up(harr[i], arr_bytes[i]); arr[i] = darr[i].p; }
    void* dptr[CIRC_NBUFS];
    for (int i = 0; i < CIRC_NBUFS && e == hipSuccess; i++) { e = dio[i].up(io[i], io_bytes[i]); dptr[i] = dio[i].p; }
    if (e == hipSuccess) e = datab.up(nullptr, circp::atab_entries(s) * sizeof(apt_packed));
    if (e == hipSuccess) e = dtscr.up(nullptr, circp::tscr_words(s) * sizeof(u32));
    if (e == hipSuccess) e = dstraus.up(nullptr, circp::straus_slots(s) * sizeof(pt_slot));
    if (e != hipSuccess) return (int)e;
    const CircuitWs r = circp::workspace(s, (const uint8_t*)in[circp::I_LABEL], dtable.p, dcom.p, dproofs.p, arr, dptr, (apt_packed*)datab.p,
                                         (u32*)dtscr.p, (pt_slot*)dstraus.p);
    const size_t n = s.N;
    const unsigned blocks = blocks_of(n);
    const bppp_host::GenericPlan& plan = s.plan;
    k_circuit_phase1<<<blocks, BPPP_BLOCK, 0, 0>>>(r);
    e = hipGetLastError();
    if (e == hipSuccess) {
        if (plan.fb == bppp_host::GENERIC_FB_WAVEFRONT) k_circuit_c0_fixed_l64<<<fb64_blocks_of(n), BPPP_FB_BLOCK, 0, 0>>>(r);
        else k_circuit_c0_fixed<<<fb_blocks_of(n), BPPP_FB_BLOCK, 0, 0>>>(r);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        if (s.form == CIRC_VAR_POINTS) {
            k_circuit_c0_var_pts<<<(unsigned)(((size_t)plan.c0_lanes * n + BPPP_BLOCK - 1) / BPPP_BLOCK), BPPP_BLOCK, 0, 0>>>(r, plan.c0_lanes);
        } else {
            if (r.atab) k_circuit_c0_tables<<<blocks, BPPP_BLOCK, 0, 0>>>(r);
            e = hipGetLastError();
            if (e == hipSuccess) k_circuit_c0_var<<<blocks, BPPP_BLOCK, 0, 0>>>(r);
        }
        if (e == hipSuccess) e = hipGetLastError();
    }
    if (e == hipSuccess) { k_circuit_c0_finish<<<blocks, BPPP_BLOCK, 0, 0>>>(r); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (int i = 0; i < CIRC_NBUFS - 1 && e == hipSuccess; i++) e = dio[i].down(io[i], io_bytes[i]);
    if (e == hipSuccess) circp::plan_words(s, (int32_t*)io[circp::B_PLAN]);
    return (int)e;
}
