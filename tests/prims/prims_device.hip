// TEST-ONLY gfx950 build of the primitive dispatcher (prims_core.h): one record per lane, compiled with the product's own flags
// (bp_pp_amd/_build.py BASE_FLAGS) by tests/prims/build.py into libbppp_prims_hip.so.
#include <hip/hip_runtime.h>

#include "prims_core.h"
#include "../../bp_pp_amd/csrc/kernels.h"     // for_each_position_group

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

// ---- the variable-base sums (prims_core.h: SumForm): a launch of n sums of one configuration.  The tables come first, in a kernel of
// their own (a lane per sum for the four-inversion builder, a lane per table for the one-lane builder of the split sums); then the sum,
// one lane per sum or G lanes per sum for the lane-group forms, so that a wavefront holds 64 / G independent sums side by side.
template <int M>
__global__ __launch_bounds__(64) void k_sum_tables(prims::SumWs w, const uint32_t* in, int parts) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (parts == 0) {
        if (tid < w.N) prims::sum_tables_build<M>(w, tid, in + tid * SUM_IN_WORDS);
        return;
    }
    const size_t s = tid / (size_t)(parts * M);
    if (s < w.N) prims::sum_table_one<M>(w, s, in + s * SUM_IN_WORDS, (int)(tid - s * (size_t)(parts * M)), parts);
}
template <int M>
__global__ __launch_bounds__(64) void k_sum_lane(prims::SumWs w, const uint32_t* in, uint32_t* out, uint32_t cfg) {
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= w.N) return;
    const uint32_t* rec = in + s * SUM_IN_WORDS;
    uint32_t* o = out + s * SUM_OUT_WORDS;
    if (rec[0] != cfg) { o[SUM_OUT_WORDS - 1] = prims::ST_BAD_PARAM; return; }
    prims::sum_one_lane<M>(cfg & 0xFFu, (int)(cfg >> 24), w, s, rec, o);
}
// PARTS = 0: straus_affine_g4<M, G>; 2, 4: straus_affine_split<M, G, PARTS>.  The G lanes of a group are consecutive lanes of one
// wavefront (G divides 64) and leave together when the group holds no sum.
template <int M, int G, int PARTS>
__global__ __launch_bounds__(64) void k_sum_group(prims::SumWs w, const uint32_t* in, uint32_t* out, uint32_t cfg) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t s = tid / G;
    const int q = (int)(tid % G);
    if (s >= w.N) return;
    const uint32_t* rec = in + s * SUM_IN_WORDS;
    uint32_t* o = out + s * SUM_OUT_WORDS;
    if (rec[0] != cfg) { if (q == 0) o[SUM_OUT_WORDS - 1] = prims::ST_BAD_PARAM; return; }
    int pidx[M];
    bppp::glv_words<M> g;
    prims::sum_scalars<M>(g, pidx, rec);
    const bppp::atab_ref tab = bppp::atab_of(w.atab, w.N, s);
    bppp::pt r, first;
    if constexpr (PARTS == 0) bppp::straus_affine_g4<M, G>(r, tab, pidx, g, q);
    else bppp::straus_affine_split<M, G, PARTS>(r, tab, pidx, g, q, M);
    // every lane of the group ends with the total: compare with lane 0's as projective points
    const int lead = (int)(threadIdx.x & 63u) - q;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        first.X.v[i] = __shfl(r.X.v[i], lead, 64);
        first.Y.v[i] = __shfl(r.Y.v[i], lead, 64);
        first.Z.v[i] = __shfl(r.Z.v[i], lead, 64);
    }
    if (!bppp::pt_eq(r, first)) atomicAdd(&o[72], 1u);
    // whether the group met an exceptional addition (and so re-did the sum completely), found again outside the function under test:
    // the split forms' lane is straus_split_lane itself; a g4 lane's additions are those of the one-lane fast sum over its own
    // streams q, q + G, ... with every other stream's half-scalar set to zero (all digits zero: skipped)
    int bad;
    bppp::pt scratch;
    if constexpr (PARTS == 0) {
        bppp::glv_words<M> mine = g;
        const bppp::u32 zero4[5] = {0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u, 0x8u};     // |k| = 0 as glv_decompose hands it over
#pragma unroll
        for (int st = 0; st < 2 * M; st++) {
            if (st % G != q) { bppp::glv_recode5(mine.w[st], zero4); mine.neg[st] = false; }
        }
        bad = bppp::straus_affine_fast<M>(scratch, tab, pidx, mine) ? 0 : 1;
    } else {
        bad = bppp::straus_split_lane<M>(scratch, tab, pidx, g, q, PARTS, M) ? 0 : 1;
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1) bad |= __shfl_xor(bad, m, 64);
    if (q == 0) { prims::sum_outputs(o, r, 2); o[73] = (uint32_t)bad; }
}

PRIMS_API int prims_sum_words(int which) { return which == 0 ? SUM_IN_WORDS : SUM_OUT_WORDS; }
template <int M>
static hipError_t sums_launch(uint32_t cfg, const prims::SumWs& w, const uint32_t* din, uint32_t* dout) {
    const uint32_t form = cfg & 0xFFu, g = (cfg >> 16) & 0xFFu, parts = cfg >> 24;
    const size_t tl = parts ? w.N * parts * M : w.N;
    hipLaunchKernelGGL(k_sum_tables<M>, dim3((unsigned)((tl + 63) / 64)), dim3(64), 0, 0, w, din, (int)parts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((w.N * g + 63) / 64));
    if (form < prims::SUM_GROUP) {
        hipLaunchKernelGGL(k_sum_lane<M>, grid, dim3(64), 0, 0, w, din, dout, cfg);
        return hipGetLastError();
    }
    // the lane-group forms the verifiers instantiate (verify_core.h, recip_core.h, wnla_core.h, prove_core.h)
    if constexpr (M == 2 || M == 5) {
        constexpr int G2 = M == 2 ? 8 : 32, G4 = M == 2 ? 16 : 64;     // groups of the split in two and in four
        if (form == prims::SUM_GROUP && g == 2) hipLaunchKernelGGL((k_sum_group<M, 2, 0>), grid, dim3(64), 0, 0, w, din, dout, cfg);
        else if (form == prims::SUM_GROUP && g == 4) hipLaunchKernelGGL((k_sum_group<M, 4, 0>), grid, dim3(64), 0, 0, w, din, dout, cfg);
        else if (form == prims::SUM_SPLIT_GROUP && parts == 2 && g == G2) hipLaunchKernelGGL((k_sum_group<M, G2, 2>), grid, dim3(64), 0, 0, w, din, dout, cfg);
        else if (form == prims::SUM_SPLIT_GROUP && parts == 4 && g == G4) hipLaunchKernelGGL((k_sum_group<M, G4, 4>), grid, dim3(64), 0, 0, w, din, dout, cfg);
        else return hipErrorInvalidValue;
        return hipGetLastError();
    }
    return hipErrorInvalidValue;
}
// n records of one configuration (cfg = prims::sum_cfg) through the table kernel and the sum kernel.  Returns the first HIP error.
PRIMS_API int prims_run_sums_device(uint32_t cfg, const uint32_t* in, uint32_t* out, size_t n) {
    if (n == 0) return 0;
    if (!prims::sum_cfg_ok(cfg)) return (int)hipErrorInvalidValue;
    const uint32_t m = (cfg >> 8) & 0xFFu, parts = cfg >> 24, np = parts ? parts : 1;
    const size_t in_sz = n * SUM_IN_WORDS * sizeof(uint32_t), out_sz = n * SUM_OUT_WORDS * sizeof(uint32_t);
    uint32_t *din = nullptr, *dout = nullptr;
    prims::SumWs w = {n, nullptr, nullptr, nullptr};
    hipError_t e = hipMalloc((void**)&din, in_sz);
    if (e == hipSuccess) e = hipMalloc((void**)&dout, out_sz);
    if (e == hipSuccess) e = hipMalloc((void**)&w.pts, n * 16 * m * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&w.tscr, n * BPPP_TSCR_PER_POINT * m * 10 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&w.atab, n * np * m * 16 * sizeof(bppp::apt_packed));
    if (e == hipSuccess) e = hipMemcpy(din, in, in_sz, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0, out_sz);
    if (e == hipSuccess) {
        switch (m) {
        case 1: e = sums_launch<1>(cfg, w, din, dout); break;
        case 2: e = sums_launch<2>(cfg, w, din, dout); break;
        case 3: e = sums_launch<3>(cfg, w, din, dout); break;
        case 4: e = sums_launch<4>(cfg, w, din, dout); break;
        default: e = sums_launch<5>(cfg, w, din, dout); break;
        }
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, out_sz, hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    if (w.pts) (void)hipFree(w.pts);
    if (w.tscr) (void)hipFree(w.tscr);
    if (w.atab) (void)hipFree(w.atab);
    return (int)e;
}

// ---- the transcript primitives (prims_core.h: TrStep): one program over n records, one record per lane, in 64-thread blocks.
// TR_UNIFORM calls the body directly: every lane of a wavefront must start at the same byte position (a wavefront that does not is
// answered with TR_BAD_LAYOUT and not run: mixed positions outside the grouping wrapper break the functions' precondition).
// TR_GROUPED runs the body inside for_each_position_group(preloaded_position_key(..)), as the product's kernels do.
struct TrProg { uint32_t w[TR_PROG_WORDS]; };
// what a lane does before its body: the program's bounds, and for the uniform layout the state and the wavefront's positions
__device__ __forceinline__ bool tr_lane_begin(const TrProg& prog, uint32_t form, uint32_t layout, const uint8_t* st, uint32_t* o) {
    if (!prims::tr_prog_ok(prog.w, form)) { o[51] = prims::ST_BAD_PARAM; return false; }
    if (layout == prims::TR_GROUPED) return true;
    if (!(st[200] < BPPP_STROBE_R && st[201] <= BPPP_STROBE_R)) { o[51] = prims::TR_BAD_STATE; return false; }
    const uint32_t pos = st[200];
    if (__any(pos != (uint32_t)__builtin_amdgcn_readfirstlane((int)pos))) { o[51] = prims::TR_BAD_LAYOUT; return false; }
    return true;
}
__global__ __launch_bounds__(64) void k_transcript_regs(TrProg prog, uint32_t layout, const uint8_t* states, const uint32_t* in, uint32_t* out,
                                                        size_t n) {
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint8_t* st = states + r * BPPP_TRANSCRIPT_STATE_BYTES;
    const uint32_t* rec = in + r * TR_IN_WORDS;
    uint32_t* o = out + r * TR_OUT_WORDS;
    if (!tr_lane_begin(prog, prims::TR_REGS, layout, st, o)) return;
    if (layout == prims::TR_UNIFORM) prims::tr_eval_regs(prog.w, st, rec, o);
    else bppp::for_each_position_group(bppp::preloaded_position_key(states, n, r), [&]() { prims::tr_eval_regs(prog.w, st, rec, o); });
}
// the LDS sponge: each lane's column is sponge + threadIdx.x (k_verify_phase1); the state goes back through ws_st_transcript's word layout
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void tr_eval_lds(const TrProg& prog, const uint8_t* st, const uint32_t* rec, uint32_t* o, uint32_t* col,
                                            uint32_t* tstate, size_t n, size_t r) {
    bppp::strobe t0;
    if (!bppp::strobe_from_bytes(t0, st)) { o[51] = prims::TR_BAD_STATE; return; }
    bppp::strobe_lds t;
    t.col = col;
    bppp::strobe_lds_load(t, t0);
    const uint32_t flags = prims::tr_run_program(t, prog.w, rec, o, st[202]);
    bppp::ws_st_transcript(tstate, n, r, t);
    bppp::strobe back;
    bppp::ws_ld_transcript(back, tstate, n, r);
    uint8_t b[204];
    b[203] = 0;
    bppp::strobe_to_bytes(b, back, flags);
    prims::st_bytes(o, b, 204);
    o[51] = prims::ST_OK;
}
#endif
__global__ __launch_bounds__(64) void k_transcript_lds(TrProg prog, uint32_t layout, const uint8_t* states, const uint32_t* in, uint32_t* out,
                                                       uint32_t* tstate, size_t n) {
    __shared__ uint32_t sponge[50 * BPPP_LDS_STRIDE];
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint8_t* st = states + r * BPPP_TRANSCRIPT_STATE_BYTES;
    const uint32_t* rec = in + r * TR_IN_WORDS;
    uint32_t* o = out + r * TR_OUT_WORDS;
    if (!tr_lane_begin(prog, prims::TR_LDS, layout, st, o)) return;
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t* col = sponge + threadIdx.x;
    if (layout == prims::TR_UNIFORM) tr_eval_lds(prog, st, rec, o, col, tstate, n, r);
    else bppp::for_each_position_group(bppp::preloaded_position_key(states, n, r), [&]() { tr_eval_lds(prog, st, rec, o, col, tstate, n, r); });
#else
    (void)sponge; (void)tstate;
#endif
}

PRIMS_API int prims_transcript_words(int which) { return which == 0 ? TR_IN_WORDS : which == 1 ? TR_OUT_WORDS : TR_PROG_WORDS; }
// n records through one program (TR_PROG_WORDS words) on one sponge form and launch layout.  Returns the first HIP error.
PRIMS_API int prims_run_transcript_device(const uint32_t* prog, uint32_t form, uint32_t layout, const uint8_t* states, const uint32_t* in,
                                          uint32_t* out, size_t n) {
    if (n == 0) return 0;
    if (form > prims::TR_LDS || layout > prims::TR_GROUPED) return (int)hipErrorInvalidValue;
    TrProg p;
    for (int i = 0; i < TR_PROG_WORDS; i++) p.w[i] = prog[i];
    const size_t st_sz = n * BPPP_TRANSCRIPT_STATE_BYTES, in_sz = n * TR_IN_WORDS * sizeof(uint32_t), out_sz = n * TR_OUT_WORDS * sizeof(uint32_t);
    const size_t ts_sz = n * 52 * sizeof(uint32_t);
    uint8_t* dstates = nullptr;
    uint32_t *din = nullptr, *dout = nullptr, *dts = nullptr;
    hipError_t e = hipMalloc((void**)&dstates, st_sz);
    if (e == hipSuccess) e = hipMalloc((void**)&din, in_sz);
    if (e == hipSuccess) e = hipMalloc((void**)&dout, out_sz);
    if (e == hipSuccess) e = hipMalloc((void**)&dts, ts_sz);
    if (e == hipSuccess) e = hipMemcpy(dstates, states, st_sz, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(din, in, in_sz, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0, out_sz);
    if (e == hipSuccess) e = hipMemset(dts, 0, ts_sz);
    if (e == hipSuccess) {
        const dim3 grid((unsigned)((n + 63) / 64));
        if (form == prims::TR_REGS) hipLaunchKernelGGL(k_transcript_regs, grid, dim3(64), 0, 0, p, layout, dstates, din, dout, n);
        else hipLaunchKernelGGL(k_transcript_lds, grid, dim3(64), 0, 0, p, layout, dstates, din, dout, dts, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, out_sz, hipMemcpyDeviceToHost);
    if (dstates) (void)hipFree(dstates);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    if (dts) (void)hipFree(dts);
    return (int)e;
}
