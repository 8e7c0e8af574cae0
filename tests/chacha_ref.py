"""Pure-Python reference of the seeded provers' draws (include/bppp.h: "Seeded provers"), independent of the library and of
bp_pp_amd/csrc/draw_core.h: the ChaCha20 block function of RFC 8439 2.1-2.3 with a 64-bit block counter (state words 12-13) and a
64-bit stream id (words 14-15) -- the rand_chacha layout -- and draw j of a stream = its block j read big-endian, mod n
(k256 Scalar::generate_biased)."""
import struct

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
_M32 = 0xFFFFFFFF


def _rotl(v: int, r: int) -> int:
    return ((v << r) | (v >> (32 - r))) & _M32


def _qr(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & _M32; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & _M32; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & _M32; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & _M32; x[b] = _rotl(x[b] ^ x[c], 7)


def block(key: bytes, counter: int, stream: int) -> bytes:
    """The 64 keystream bytes of block `counter` (u64) of stream `stream` (u64) under the 32-byte key."""
    assert len(key) == 32 and 0 <= counter < 1 << 64 and 0 <= stream < 1 << 64
    st = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574, *struct.unpack("<8I", key),
          counter & _M32, counter >> 32, stream & _M32, stream >> 32]
    x = list(st)
    for _ in range(10):
        _qr(x, 0, 4, 8, 12); _qr(x, 1, 5, 9, 13); _qr(x, 2, 6, 10, 14); _qr(x, 3, 7, 11, 15)
        _qr(x, 0, 5, 10, 15); _qr(x, 1, 6, 11, 12); _qr(x, 2, 7, 8, 13); _qr(x, 3, 4, 9, 14)
    return struct.pack("<16I", *((a + b) & _M32 for a, b in zip(x, st)))


def rfc_block(key: bytes, counter32: int, nonce12: bytes) -> bytes:
    """RFC 8439's own layout (32-bit counter, 96-bit nonce) expressed in the 64/64 one: the same 16 state words."""
    w13, w14, w15 = struct.unpack("<3I", nonce12)
    return block(key, counter32 | (w13 << 32), w14 | (w15 << 32))


def draw(seed: bytes, stream: int, j: int) -> int:
    """Draw j of stream `stream`: block j big-endian mod n."""
    return int.from_bytes(block(seed, j, stream), "big") % N


def draws(seed: bytes, stream_base: int, n: int, k: int) -> bytes:
    """n x k x 32 bytes: instance i's draws from stream stream_base + i, the provers' `rnd` layout."""
    return b"".join(draw(seed, stream_base + i, j).to_bytes(32, "big") for i in range(n) for j in range(k))
