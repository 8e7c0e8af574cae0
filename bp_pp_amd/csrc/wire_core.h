// Wire form of the generic proofs (reciprocal, circuit, WNLA): SEC1-compressed points <-> the 64-byte x||y form of the C ABI, for any
// layout.  The reference's SerializableProof types (reciprocal.rs:37-41, circuit.rs:36-46, wnla.rs:33-38) hold k256 `AffinePoint`s; their
// byte form is the C-ABI layout with every point compressed in place (33 bytes: 02|03 || x, the identity 33 zero bytes) and the scalars
// copied.  A WireMap describes one call's conversion as up to BPPP_WIRE_SEGS segments, each `count` points (or 32-byte scalars) per
// instance at a per-instance stride on either side, so that the same two kernels serve a contiguous proof (the verifiers' input) and the
// separate arrays a prover leaves behind (head, r, x, reciprocal r, l, n).
//
// Lanes: one per point over the flat batch, segment after segment (sum over the point segments of n * count lanes: no idle lane but in
// the tail), then one per 4-byte word of the scalar segments.  The 64-byte side is always the library's own buffer (4-byte aligned: every
// stride and offset there is a multiple of 32); the 33-byte side has no alignment and is read / written byte-wise.
#pragma once
#include "verify_core.h"

namespace bppp {

#define BPPP_WIRE_SEGS 8

struct WireSeg {
    const uint8_t* src;          // instance 0's first element (33-byte side for expand, 64-byte side for compress)
    uint8_t* dst;
    size_t src_stride, dst_stride;      // bytes from one instance to the next
    u32 count;                   // points or scalars per instance
    u32 scalar;                  // 0: points (decompress / compress), 1: 32-byte scalars (copied word by word)
};
struct WireMap {
    WireSeg seg[BPPP_WIRE_SEGS];
    u64 first[BPPP_WIRE_SEGS + 1];      // first lane of each segment; first[nseg] = lanes of the call
    int nseg;
    size_t n;
    const int32_t* zero_if;      // compress only (may be null): an instance whose status is nonzero comes out as zero bytes
};

// host side: a segment (empty ones are dropped), then wire_map_finish: point segments first, lane offsets
HD void wire_map_init(WireMap& m, size_t n) {
    m.nseg = 0;
    m.n = n;
    m.zero_if = nullptr;
}
HD bool wire_map_add(WireMap& m, bool scalar, const uint8_t* src, size_t src_stride, uint8_t* dst, size_t dst_stride, size_t count) {
    if (count == 0) return true;
    if (m.nseg == BPPP_WIRE_SEGS) return false;
    WireSeg& s = m.seg[m.nseg++];
    s.src = src; s.dst = dst; s.src_stride = src_stride; s.dst_stride = dst_stride; s.count = (u32)count; s.scalar = scalar ? 1u : 0u;
    return true;
}
HD u64 wire_map_finish(WireMap& m) {
    WireSeg tmp[BPPP_WIRE_SEGS];
    int k = 0;
    for (int pass = 0; pass < 2; pass++)
        for (int i = 0; i < m.nseg; i++)
            if ((int)m.seg[i].scalar == pass) tmp[k++] = m.seg[i];
    u64 lanes = 0;
    for (int i = 0; i < m.nseg; i++) {
        m.seg[i] = tmp[i];
        m.first[i] = lanes;
        lanes += (u64)m.n * m.seg[i].count * (m.seg[i].scalar ? 8u : 1u);
    }
    m.first[m.nseg] = lanes;
    return lanes;
}

// lane g -> (segment, instance, element or word).  The segment is picked by an unrolled select, not by a dynamic index into the
// kernel argument (which the compiler would copy to scratch memory to index)
HD WireSeg wire_locate(const WireMap& m, u64 g, size_t& t, u32& j) {
    WireSeg sg = m.seg[0];
    u64 f = m.first[0];
#pragma unroll
    for (int i = 1; i < BPPP_WIRE_SEGS; i++)
        if (i < m.nseg && g >= m.first[i]) {
            sg = m.seg[i];
            f = m.first[i];
        }
    const u64 per = (u64)sg.count * (sg.scalar ? 8u : 1u);
    const u64 q = g - f;
    t = (size_t)(q / per);
    j = (u32)(q - (u64)t * per);
    return sg;
}

// 33-byte side -> 64-byte side: a point through sec1_decompress_to_xy64 (an undecodable one becomes the off-curve (1, 0), which the
// verifiers' phase 1 and the provers' input checks flag BPPP_ST_BAD_ENCODING), a scalar word as it is
HD void wire_expand_lane(const WireMap& m, u64 g) {
    size_t t;
    u32 j;
    const WireSeg sg = wire_locate(m, g, t, j);
    if (!sg.scalar) {
        sec1_decompress_to_xy64(sg.dst + t * sg.dst_stride + 64 * (size_t)j, sg.src + t * sg.src_stride + 33 * (size_t)j);
    } else {
        const uint8_t* in = sg.src + t * sg.src_stride + 4 * (size_t)j;
        const u32 v = (u32)in[0] | ((u32)in[1] << 8) | ((u32)in[2] << 16) | ((u32)in[3] << 24);
        *(u32*)(sg.dst + t * sg.dst_stride + 4 * (size_t)j) = v;
    }
}

// 64-byte side -> 33-byte side: tag 02 / 03 by the parity of y, the identity (64 zero bytes) -> 33 zero bytes (as sec1_compress_lane);
// the 64-byte points are the library's own output (canonical, on the curve)
HD void wire_compress_lane(const WireMap& m, u64 g) {
    size_t t;
    u32 j;
    const WireSeg sg = wire_locate(m, g, t, j);
    const bool zero = m.zero_if && m.zero_if[t] != 0;
    if (!sg.scalar) {
        const u32* in = (const u32*)(sg.src + t * sg.src_stride + 64 * (size_t)j);
        uint8_t* out = sg.dst + t * sg.dst_stride + 33 * (size_t)j;
        u32 w[16];
        u32 any = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            w[i] = zero ? 0u : in[i];
            any |= w[i];
        }
        out[0] = any ? (uint8_t)(2 + ((w[15] >> 24) & 1)) : (uint8_t)0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            out[1 + 4 * i] = (uint8_t)w[i];
            out[2 + 4 * i] = (uint8_t)(w[i] >> 8);
            out[3 + 4 * i] = (uint8_t)(w[i] >> 16);
            out[4 + 4 * i] = (uint8_t)(w[i] >> 24);
        }
    } else {
        const u32 v = zero ? 0u : *(const u32*)(sg.src + t * sg.src_stride + 4 * (size_t)j);
        uint8_t* out = sg.dst + t * sg.dst_stride + 4 * (size_t)j;
        out[0] = (uint8_t)v;
        out[1] = (uint8_t)(v >> 8);
        out[2] = (uint8_t)(v >> 16);
        out[3] = (uint8_t)(v >> 24);
    }
}

}  // namespace bppp
