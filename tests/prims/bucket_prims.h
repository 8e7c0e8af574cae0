// TEST-ONLY: what the two builds of the bucket-stage entry point share (prims_host.cpp: prims_run_bucket_host, the single-thread form of
// bucket_core.h; bucket_device.hip: prims_run_bucket_device, the product's k_bkt_* kernels).  tests/test_prims_bucket.py calls both with
// plain arrays and compares every output with big integers.
//
//   N, M, nb       proofs, proofs per superchunk (1 .. BPPP_BKT_MAX_M), bases (1 .. BKT_MAX_NB); ns = ceil(N / M) superchunks
//   seed[4]        the weights' key | status[N] | acc [30][N] projective limbs of C_j | fsc [nb * 8][N] scalars s_ji
//   table, W       fixed-base table of the nb bases (prims_bucket_fb_build), W = 4
//   given          0: wab and c4 come from bkt_prepare; 1: the caller's wab and c4 are used as they are (crafted digits)
//   wab [N][2], c4 [N][24] (x, y, z as 8 words each), lhs [30][ns], asc [nb * 8][ns], sflag [ns], accept [N]: outputs; sflag and accept
//   are filled with BKT_SENTINEL before anything runs, so a byte nothing wrote still holds it
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../bp_pp_amd/csrc/bucket_core.h"

#define BKT_SENTINEL 0xA5
#define BKT_MAX_NB 1024
#define BKT_MAX_N ((size_t)1 << 20)

namespace bktp {

inline bool args_ok(size_t N, uint32_t M, int nb, int W) {
    return N >= 1 && N <= BKT_MAX_N && M >= 1 && M <= BPPP_BKT_MAX_M && nb >= 1 && nb <= BKT_MAX_NB && W == 4;
}
inline size_t nsuper_of(size_t N, uint32_t M) { return (N + M - 1) / M; }
inline size_t fb_entries(int nb, int W) { return (size_t)nb * bppp::fb_per_base(W); }

// The table of nb generators (64-byte affine x | y each) by the product's two construction passes, two bases at a time as the library
// does for tables too large to build at once.  table_out: fb_entries(nb, W) x 64 B.  Returns 0, or -1 for a generator off the curve.
inline int fb_build(const uint8_t* gens, int nb, int W, uint8_t* table_out) {
    using namespace bppp;
    std::vector<apt> g((size_t)nb);
    for (int i = 0; i < nb; i++)
        if (!apt_from_xy64(g[(size_t)i], gens + 64 * i)) return -1;
    const size_t per_base = fb_per_base(W), group = 2, gentries = group * per_base;
    std::vector<fe> tmp(gentries * 4);
    for (int b0 = 0; b0 < nb; b0 += (int)group) {
        const int cnt = nb - b0 < (int)group ? nb - b0 : (int)group;
        FbBuild fb{g.data(), nb, W, (apt_packed*)table_out, tmp.data(), tmp.data() + gentries, tmp.data() + 2 * gentries,
                   tmp.data() + 3 * gentries, b0, cnt, 0};
        const size_t nthreads = (size_t)cnt * (size_t)fb_nwin(W) * fb_chunks_per_window(W);
        for (size_t t = 0; t < nthreads; t++) fb_build_pass1(fb, t);
        for (size_t t = 0; t < nthreads; t++) fb_build_pass2(fb, t);
    }
    return 0;
}

// the workspace over caller-visible arrays (host build: the arrays themselves; device build: their device copies)
inline bppp::BucketWs workspace(size_t N, uint32_t M, int nb, const uint64_t seed[4], const int32_t* status, const uint32_t* acc,
                                const uint32_t* fsc, const uint8_t* table, int W, uint64_t* wab, uint32_t* c4, uint32_t* lhs, uint32_t* asc,
                                uint8_t* sflag, uint8_t* accept) {
    bppp::BucketWs w = {};
    w.N = N; w.M = M; w.nb = nb;
    for (int i = 0; i < 4; i++) w.seed[i] = seed[i];
    w.status = status; w.acc = acc; w.fsc = fsc;
    w.wab = (bppp::u64*)wab; w.c4 = (bppp::c4_packed*)c4; w.lhs = lhs; w.asc = asc; w.sflag = sflag; w.accept = accept;
    w.fb.table = (const bppp::apt_packed*)table; w.fb.W = W; w.fb.N = nsuper_of(N, M);
    return w;
}

}  // namespace bktp
