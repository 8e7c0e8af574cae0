// The seeded provers' random scalars: ChaCha20 blocks reduced mod n, one draw per block (include/bppp.h: "Seeded provers").
//
// Instance i of a call with seed (32 bytes) and stream_base draws j = 0 .. k-1 as
//   block  = ChaCha20 block function, 20 rounds (RFC 8439 2.1-2.3); state words 0-3 the constants, 4-11 the key = seed as
//            little-endian words, 12-13 the 64-bit block counter j (low, high), 14-15 the 64-bit stream stream_base + i (low, high)
//   draw_j = the block's 64 output bytes read as a big-endian integer, mod n      (k256 Scalar::generate_biased)
// which is what `ChaCha20Rng::from_seed(seed)` + `set_stream(stream_base + i)` followed by k calls of `generate_biased` gives: every
// 64-byte request takes exactly one block.
//
// Host and device code with no HIP in it (like merlin.h): libbppp_hip.so's host entry point (bppp_draw_scalars), its kernel
// (k_draw.hip: k_draw_scalars) and the CPU tier's g++ shim (tests/test_draw.py) compile this same file.
//
// Constant time: no branch and no address depends on the seed or on a draw.  The block function is a fixed sequence of adds, xors and
// rotates; the reduction is three folds by 2^256 - n whose count follows from fixed bounds, then one subtraction of n selected by mask.
#pragma once
#include "field.h"

namespace bppp {

// rotate left by a compile-time amount: one v_alignbit_b32 on gfx950 ({v, v} >> (32 - r))
HD u32 draw_rotl(u32 v, int r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(v, v, (u32)(32 - r));
#else
    return (v << r) | (v >> (32 - r));
#endif
}
HD u32 draw_bswap(u32 v) { return __builtin_bswap32(v); }   // v_perm_b32 on gfx950

HD void chacha_qr(u32& a, u32& b, u32& c, u32& d) {
    a += b; d ^= a; d = draw_rotl(d, 16);
    c += d; b ^= c; b = draw_rotl(b, 12);
    a += b; d ^= a; d = draw_rotl(d, 8);
    c += d; b ^= c; b = draw_rotl(b, 7);
}

// the 32-byte seed as the eight little-endian key words (a kernel argument of k_draw_scalars: it never sits in device memory)
struct DrawKey { u32 w[8]; };
HD void chacha_key(u32 key[8], const uint8_t seed[32]) {
#pragma unroll
    for (int i = 0; i < 8; i++)
        key[i] = (u32)seed[4 * i] | ((u32)seed[4 * i + 1] << 8) | ((u32)seed[4 * i + 2] << 16) | ((u32)seed[4 * i + 3] << 24);
}

// RFC 8439 2.3 with a 64-bit counter and a 64-bit stream id (the rand_chacha layout): out = the 16 little-endian output words
HD void chacha20_block(u32 out[16], const u32 key[8], u64 counter, u64 stream) {
    u32 in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3], key[4], key[5], key[6], key[7],
                  (u32)counter, (u32)(counter >> 32), (u32)stream, (u32)(stream >> 32)};
    u32 x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = in[i];
#pragma unroll
    for (int r = 0; r < 10; r++) {
        chacha_qr(x[0], x[4], x[8], x[12]);
        chacha_qr(x[1], x[5], x[9], x[13]);
        chacha_qr(x[2], x[6], x[10], x[14]);
        chacha_qr(x[3], x[7], x[11], x[15]);
        chacha_qr(x[0], x[5], x[10], x[15]);
        chacha_qr(x[1], x[6], x[11], x[12]);
        chacha_qr(x[2], x[7], x[8], x[13]);
        chacha_qr(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = x[i] + in[i];
}

// t (16 little-endian 32-bit limbs, any 512-bit value) mod n -> r (8 limbs, canonical).
//   fold 1: t_lo + t_hi ND           < 2^256 + 2^385            (13 limbs; ND = 2^256 - n < 2^129)
//   fold 2: a_lo + a[8..13) ND       < 2^256 + 2^130 2^129      ( 9 limbs: a[8..13) < 2^130)
//   fold 3: b_lo + b[8] ND           < 2^256 + 2^134            (b[8] < 2^5, so at most one more 2^256 in d[8])
//   then the value d_lo + d[8] 2^256 is below 2n, and one subtraction of n (adding ND mod 2^256) is selected by mask.
HD void draw_reduce512(u32 r[8], const u32 t[16]) {
    u32 a[13];
    sc_fold<8>(a, t, t + 8);
    u32 b[10];
    sc_fold<5>(b, a, a + 8);
    const u32 nd5[5] = {BPPP_ND0, BPPP_ND1, BPPP_ND2, BPPP_ND3, BPPP_ND4};
    u32 d[9];
    {
        const u32 h = b[8];
        u64 p[5];
#pragma unroll
        for (int j = 0; j < 5; j++) p[j] = (u64)h * nd5[j];
        u32 cy = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) d[i] = addc(i < 8 ? b[i] : 0u, i < 5 ? (u32)p[i] : 0u, cy);
        cy = 0;
#pragma unroll
        for (int i = 1; i < 9; i++) d[i] = addc(d[i], (i - 1) < 5 ? (u32)(p[i - 1] >> 32) : 0u, cy);
    }
    // value >= n  <=>  d[8] = 1, or d_lo + ND carries out of 2^256; then value - n = d_lo + ND mod 2^256
    u32 e[8];
    u32 c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = addc(d[i], i < 5 ? nd5[i] : 0u, c);
    const u32 take = 0u - ((d[8] | c) & 1u);
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = d[i] ^ ((d[i] ^ e[i]) & take);
}

// one draw: block `counter` of stream `stream` reduced mod n, as the 8 little-endian words of its 32 big-endian bytes (memory order)
HD void draw_scalar_words(u32 out[8], const u32 key[8], u64 stream, u64 counter) {
    u32 blk[16];
    chacha20_block(blk, key, counter, stream);
    // the block's bytes big-endian: the least significant limb is the last output word, byte-swapped
    u32 t[16];
#pragma unroll
    for (int i = 0; i < 16; i++) t[i] = draw_bswap(blk[15 - i]);
    u32 r[8];
    draw_reduce512(r, t);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = draw_bswap(r[7 - i]);
}

}  // namespace bppp
