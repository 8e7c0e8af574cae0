"""Generates tests/golden/chacha20_openssl.json with the OpenSSL command-line tool (`openssl enc -chacha20`, 3.0.2 in this image):
a ChaCha20 that shares nothing with this repository, to pin the block function of the seeded provers' draws (include/bppp.h:
"Seeded provers").  OpenSSL takes a 16-byte IV = 32-bit little-endian block counter || 96-bit nonce; block j (< 2^32) of 64-bit
stream s in the rand_chacha layout (state words 12-13 the counter, 14-15 the stream) is therefore the keystream of IV
le32(j) || 00000000 || le64(s).  Only the keystream bytes are committed.
Run:  python tests/golden/make_chacha_vectors.py"""
import hashlib
import json
import os
import struct
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def openssl_block(key: bytes, j: int, stream: int) -> bytes:
    iv = struct.pack("<IIQ", j, 0, stream)
    r = subprocess.run(["openssl", "enc", "-chacha20", "-K", key.hex(), "-iv", iv.hex(), "-nosalt"], input=bytes(64),
                       capture_output=True, check=True)
    assert len(r.stdout) == 64
    return r.stdout


def main():
    seeds = [bytes(32), bytes(range(32)), hashlib.sha256(b"bppp seeded prover vectors").digest(), b"\xff" * 32]
    streams = [0, 1, 0x4A000000, (1 << 32) - 2, (1 << 32) + 7, 0x0123456789ABCDEF, (1 << 64) - 1]
    blocks = [0, 1, 51, 52, 531, 600]
    cases = []
    for si, seed in enumerate(seeds):
        for ti, stream in enumerate(streams):
            j = blocks[(si + ti) % len(blocks)]
            for jj in sorted({j, blocks[(si * 3 + ti * 5 + 1) % len(blocks)]}):
                cases.append({"seed": seed.hex(), "stream": str(stream), "block": jj, "keystream": openssl_block(seed, jj, stream).hex()})
    out = {"source": subprocess.run(["openssl", "version"], capture_output=True, text=True).stdout.strip(),
           "iv_layout": "le32(block) || 00000000 || le64(stream)", "cases": cases}
    with open(os.path.join(HERE, "chacha20_openssl.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(len(cases), "cases")


if __name__ == "__main__":
    main()
