// Wire form of aggregated reciprocal range proofs of MIXED value counts (agg_mixed_core.h): the 33-byte slots of a call to its 64-byte
// slots, both laid out by k_max.  Instance t carries k_t = ks[t] values: its commitments are the first k_t of its k_max slots, its proof
// the first 33 (4 + 2 rounds + k_t) + 32 (nl + nn) bytes of its slot in the uniform wire layout for k_t -- 4 + 2 rounds + k_t compressed
// points, then l | n.  It comes out in the 64-byte layout for k_t: points at 64 j, l | n at 64 (4 + 2 rounds + k_t).  A WireMap
// (wire_core.h) cannot say this: its segments have one point count and one scalar offset for the whole call.
//
// Lanes: one per point SLOT of the k_max layout (k_max commitment slots, then 4 + 2 rounds + k_max proof slots per instance), then one
// per 4-byte word of l | n.  A point lane at or behind its instance's own count does nothing; nothing behind an instance's bytes is
// read or written on either side.  A ks[t] outside [1, k_max] is expanded as a one-value instance (agg_mixed_k's rule), so that the
// bytes phase 1 reads of such a row are defined and nothing outside the slot is touched.
// The 64-byte side is the library's own buffer (4-byte aligned; every stride and offset there is a multiple of 32); the 33-byte side
// has no alignment and is read byte-wise.
#pragma once
#include "verify_core.h"

namespace bppp {

struct WireMixed {
    const uint8_t* com33;            // [n][k_max][33]
    const uint8_t* proofs33;         // [n][33 (4 + 2 rounds + k_max) + 32 ns]
    uint8_t* com64;                  // [n][k_max][64]
    uint8_t* proofs64;               // [n][64 (4 + 2 rounds + k_max) + 32 ns]
    const uint8_t* ks;               // [n] value counts
    size_t n;
    u32 k_max, rounds, ns;           // ns = nl + nn scalars
};

HD u32 wire_mixed_points(const WireMixed& m, u32 k) { return 4 + 2 * m.rounds + k; }
// lanes of a call: the commitment slots, the proof's point slots, the scalar words
HD u64 wire_mixed_lanes(const WireMixed& m) {
    return (u64)m.n * m.k_max + (u64)m.n * wire_mixed_points(m, m.k_max) + (u64)m.n * 8 * m.ns;
}
// k_t, or 1 where ks[t] is not a value count of this call (agg_mixed_k)
HD u32 wire_mixed_k(const WireMixed& m, size_t t) {
    const u32 k = m.ks[t];
    return k < 1 || k > m.k_max ? 1u : k;
}

// a point through sec1_decompress_to_xy64 (an undecodable one becomes the off-curve (1, 0), which phase 1 flags BPPP_ST_BAD_ENCODING),
// a scalar word as it is
HD void wire_mixed_expand_lane(const WireMixed& m, u64 g) {
    const u32 PM = wire_mixed_points(m, m.k_max);
    const u64 n_com = (u64)m.n * m.k_max, n_pts = (u64)m.n * PM;
    const size_t b33 = (size_t)33 * PM + (size_t)32 * m.ns, b64 = (size_t)64 * PM + (size_t)32 * m.ns;      // the slots' strides
    if (g < n_com) {
        const size_t t = (size_t)(g / m.k_max);
        const u32 j = (u32)(g - (u64)t * m.k_max);
        if (j >= wire_mixed_k(m, t)) return;
        const size_t slot = t * m.k_max + j;
        sec1_decompress_to_xy64(m.com64 + 64 * slot, m.com33 + 33 * slot);
    } else if (g < n_com + n_pts) {
        const u64 q = g - n_com;
        const size_t t = (size_t)(q / PM);
        const u32 j = (u32)(q - (u64)t * PM);
        if (j >= wire_mixed_points(m, wire_mixed_k(m, t))) return;
        sec1_decompress_to_xy64(m.proofs64 + t * b64 + 64 * (size_t)j, m.proofs33 + t * b33 + 33 * (size_t)j);
    } else {
        const u64 q = g - n_com - n_pts;
        const u32 per = 8 * m.ns;
        const size_t t = (size_t)(q / per);
        const u32 j = (u32)(q - (u64)t * per);
        const size_t P = wire_mixed_points(m, wire_mixed_k(m, t));       // l | n sits behind this instance's own points
        const uint8_t* in = m.proofs33 + t * b33 + 33 * P + 4 * (size_t)j;
        const u32 v = (u32)in[0] | ((u32)in[1] << 8) | ((u32)in[2] << 16) | ((u32)in[3] << 24);
        *(u32*)(m.proofs64 + t * b64 + 64 * P + 4 * (size_t)j) = v;
    }
}

}  // namespace bppp
