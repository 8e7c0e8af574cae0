"""CPU tier of the seeded provers' draws (include/bppp.h: "Seeded provers"; bp_pp_amd/csrc/draw_core.h).

The ChaCha20 block function is pinned to RFC 8439 (2.3.2 and the Appendix A.1 keystream vectors) and to OpenSSL
(tests/golden/chacha20_openssl.json); the reduction to the oracle's wide_reduce.  bppp_draw_scalars (libbppp_hip.so, no GPU) must
equal the pure-Python reference (tests/chacha_ref.py), and draw_core.h built with g++ -- once more under AddressSanitizer and
UBSan where libasan exists -- must reduce chosen 512-bit inputs exactly, including the ones whose folds carry."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import chacha_ref as R  # noqa: E402
from bppp_oracle import wide_reduce  # noqa: E402

N = R.N
ND = (1 << 256) - N
SEED = bytes.fromhex("6a09e667f3bcc908bb67ae8584caa73b3c6ef372fe94f82ba54ff53a5f1d36f1")
with open(os.path.join(ROOT, "tests", "golden", "chacha20_openssl.json")) as _f:
    OPENSSL = json.load(_f)["cases"]


def _lib():
    from bp_pp_amd import _build, _capi
    if not os.path.exists(_build.SO):
        pytest.skip("libbppp_hip.so not built yet (python -c 'import __graft_entry__ as g; g.build()')")
    return _capi


# ---------------------------------------------------------------- the reference itself
def test_reference_rfc8439_block_function():
    # 2.3.2: key 00..1f, nonce 000000090000004a00000000, counter 1 = counter 0x09000000_00000001, stream 0x4a000000 in the 64/64 layout
    out = "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4ed2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e"
    assert R.rfc_block(bytes(range(32)), 1, bytes.fromhex("000000090000004a00000000")).hex() == out
    assert R.block(bytes(range(32)), 0x09000000_00000001, 0x4A000000).hex() == out


@pytest.mark.parametrize("key,counter,nonce,out", [
    (bytes(32), 0, bytes(12), "76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7da41597c5157488d7724e03fb8d84a376a43b8f41518a11cc387b669b2ee6586"),
    (bytes(32), 1, bytes(12), "9f07e7be5551387a98ba977c732d080dcb0f29a048e3656912c6533e32ee7aed29b721769ce64e43d57133b074d839d531ed1f28510afb45ace10a1f4b794d6f"),
    (bytes(31) + b"\x01", 1, bytes(12), "3aeb5224ecf849929b9d828db1ced4dd832025e8018b8160b82284f3c949aa5a8eca00bbb4a73bdad192b5c42f73f2fd4e273644c8b36125a64addeb006c13a0"),
    (b"\x00\xff" + bytes(30), 2, bytes(12), "72d54dfbf12ec44b362692df94137f328fea8da73990265ec1bbbea1ae9af0ca13b25aa26cb4a648cb9b9d1be65b2c0924a66c54d545ec1b7374f4872e99f096"),
    (bytes(32), 0, bytes(11) + b"\x02", "c2c64d378cd536374ae204b9ef933fcd1a8b2288b3dfa49672ab765b54ee27c78a970e0e955c14f3a88e741b97c286f75f8fc299e8148362fa198a39531bed6d"),
])
def test_reference_rfc8439_appendix_a1(key, counter, nonce, out):
    assert R.rfc_block(key, counter, nonce).hex() == out


def test_reference_matches_openssl_fixture():
    assert len(OPENSSL) >= 24
    assert any(int(c["stream"]) >= 1 << 32 for c in OPENSSL) and any(int(c["stream"]) == (1 << 64) - 1 for c in OPENSSL)
    assert max(c["block"] for c in OPENSSL) >= 600
    for c in OPENSSL:
        assert R.block(bytes.fromhex(c["seed"]), c["block"], int(c["stream"])).hex() == c["keystream"], c


# ---------------------------------------------------------------- bppp_draw_scalars (the library's host form)
def _draw(seed, stream_base, n, k):
    _capi = _lib()
    out = np.zeros((n, k, 32), np.uint8)
    assert _capi.lib().bppp_draw_scalars(seed, stream_base, n, k, out.ctypes.data) == _capi.OK
    return out


def _sample(m, full):
    return list(range(m)) if m <= full else sorted({0, 1, m // 2 - 1, m // 2, m - 2, m - 1, 51 % m, 52 % m, 255 % m, 256 % m})


@pytest.mark.parametrize("n", [1, 3, 1000])
@pytest.mark.parametrize("k", [1, 52, 532])
@pytest.mark.parametrize("base", ["zero", "2^32-2", "2^64-n"])
def test_draw_scalars_match_reference(n, k, base):
    stream_base = {"zero": 0, "2^32-2": (1 << 32) - 2, "2^64-n": (1 << 64) - n}[base]
    out = _draw(SEED, stream_base, n, k)
    for i in _sample(n, 3):
        for j in _sample(k, 52):
            want = R.draw(SEED, stream_base + i, j)
            assert int.from_bytes(out[i, j].tobytes(), "big") == want, (i, j)
            assert want == wide_reduce(R.block(SEED, j, stream_base + i))
    # every row is its own stream: row i of the batch = the single-instance call at stream_base + i; a shorter k is a prefix
    for i in _sample(n, 3):
        assert (_draw(SEED, stream_base + i, 1, k)[0] == out[i]).all()
    assert (_draw(SEED, stream_base, n, 1)[:, 0] == out[:, 0]).all()
    assert all(int.from_bytes(r.tobytes(), "big") < N for r in out.reshape(-1, 32)[:64])


def test_draw_scalars_match_openssl_fixture():
    for c in OPENSSL:
        seed, stream, j = bytes.fromhex(c["seed"]), int(c["stream"]), c["block"]
        got = _draw(seed, stream, 1, j + 1)[0, j].tobytes()
        assert int.from_bytes(got, "big") == wide_reduce(bytes.fromhex(c["keystream"])), c


def test_draw_scalars_invalid_arguments():
    _capi = _lib()
    L = _capi.lib()
    out = np.zeros((4, 2, 32), np.uint8)
    E = _capi.ERR_INVALID_ARG
    top = (1 << 64) - 1
    assert L.bppp_draw_scalars(SEED, top, 2, 2, out.ctypes.data) == E          # streams top, top + 1: overflow
    assert L.bppp_draw_scalars(SEED, top - 2, 4, 2, out.ctypes.data) == E
    assert L.bppp_draw_scalars(SEED, top - 3, 4, 2, out.ctypes.data) == _capi.OK  # ... top - 3 .. top: the last valid range
    assert L.bppp_draw_scalars(SEED, top, 1, 2, out.ctypes.data) == _capi.OK
    assert L.bppp_draw_scalars(None, 0, 1, 1, out.ctypes.data) == E
    assert L.bppp_draw_scalars(SEED, 0, 1, 1, None) == E
    assert L.bppp_draw_scalars_device(None, SEED, 0, 1, 1, out.ctypes.data) == E   # no context
    # the Python wrapper checks before the C call
    import bp_pp_amd
    with pytest.raises(ValueError):
        bp_pp_amd.draw_scalars(SEED[:31], 0, 1, 1)
    with pytest.raises(ValueError):
        bp_pp_amd.draw_scalars(SEED, top, 2, 1)
    assert (bp_pp_amd.draw_scalars(SEED, 5, 2, 3) == _draw(SEED, 5, 2, 3)).all()


def test_seeded_entry_points_refuse_bad_arguments_without_a_gpu():
    _capi = _lib()
    L = _capi.lib()
    E = _capi.ERR_INVALID_ARG
    buf = np.zeros(1 << 16, np.uint8)
    p = buf.ctypes.data
    assert L.bppp_u64_prove_batch_seeded(None, b"x", 1, 1, p, p, SEED, 0, p, p, p) == E
    assert L.bppp_u64_prove_batch_seeded_device(None, b"x", 1, 1, p, p, SEED, 0, p, p, p) == E
    assert L.bppp_u64_prove_batch_seeded_sharded(None, b"x", 1, 1, p, p, SEED, 0, p, p, p) == E
    assert L.bppp_reciprocal_prove_batch_seeded(None, b"x", 1, 1, 16, 16, p, p, p, p, p, SEED, 0, p, p) == E
    assert L.bppp_circuit_prove_batch_seeded(None, None, b"x", 1, 1, p, p, p, p, p, p, SEED, 0, p, p) == E


# ---------------------------------------------------------------- draw_core.h under g++ (and ASan + UBSan)
SHIM = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "draw_core.h"
using namespace bppp;
static void unhex(uint8_t* out, const char* h, int n) {
    for (int i = 0; i < n; i++) { unsigned v; std::sscanf(h + 2 * i, "%2x", &v); out[i] = (uint8_t)v; }
}
int main() {
    static char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        if (line[0] == 'R') {               // R <128 hex: a 512-bit big-endian integer>  ->  mod n, 64 hex
            uint8_t b[64];
            unhex(b, line + 2, 64);
            u32 t[16], r[8];
            for (int i = 0; i < 16; i++)
                t[i] = ((u32)b[60 - 4 * i] << 24) | ((u32)b[61 - 4 * i] << 16) | ((u32)b[62 - 4 * i] << 8) | b[63 - 4 * i];
            draw_reduce512(r, t);
            for (int i = 7; i >= 0; i--) std::printf("%08x", r[i]);
            std::printf("\n");
        } else if (line[0] == 'D') {        // D <64 hex seed> <stream> <block>  ->  the draw, 64 hex
            uint8_t seed[32];
            unhex(seed, line + 2, 32);
            unsigned long long stream = 0, j = 0;
            std::sscanf(line + 67, "%llu %llu", &stream, &j);
            u32 key[8], w[8];
            chacha_key(key, seed);
            draw_scalar_words(w, key, stream, j);
            uint8_t o[32];
            std::memcpy(o, w, 32);
            for (int i = 0; i < 32; i++) std::printf("%02x", o[i]);
            std::printf("\n");
        }
    }
    return 0;
}
'''


def _fold_trace(x):
    """The reduction's folds (draw_core.h: draw_reduce512) on integers: which final path the input takes, with its bounds checked."""
    lo, hi = x & ((1 << 256) - 1), x >> 256
    a = lo + hi * ND
    assert a < (1 << 256) + (1 << 385)
    b = (a & ((1 << 256) - 1)) + (a >> 256) * ND
    assert b >> 256 < 32
    d = (b & ((1 << 256) - 1)) + (b >> 256) * ND
    d8, dlo = d >> 256, d & ((1 << 256) - 1)
    assert d8 in (0, 1)
    c = (dlo + ND) >> 256
    return "wrap" if d8 else ("sub" if c else "keep")


def _chosen_inputs():
    xs = [0, 1, N - 1, N, N + 1, 2 * N - 1, 2 * N, (1 << 256) - 1, 1 << 256, (1 << 512) - 1, (1 << 511), ND, ND - 1]
    kmax = ((1 << 512) - 2) // N
    for k in (2, 3, 7, 1 << 64, 1 << 128, (1 << 255) + 12345, kmax):
        xs += [k * N - 1, k * N, k * N + 1]
    # inputs whose last fold carries out of 2^256 ("wrap"): fold 1 leaves a_hi = A, a_lo = B with B + (A ND mod 2^256) = 2^256 - 1 - e
    for A in ((1 << 128) - 5, (1 << 128) - 1, 3 << 126):
        for e in (0, 1, 1000):
            q, r = divmod(A * ND, 1 << 256)
            B = ((1 << 256) - 1 - e - r) % (1 << 256)
            target = A * (1 << 256) + B
            H = target // ND
            L = target - H * ND
            if 0 <= L < 1 << 256 and H < 1 << 256:
                xs.append(H * (1 << 256) + L)
    rng = np.random.default_rng(7)
    xs += [int.from_bytes(rng.bytes(64), "big") for _ in range(200)]
    return xs


def _build_shim(tmp_path, sanitize):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    src = tmp_path / "draw_shim.cpp"
    src.write_text(SHIM)
    exe = tmp_path / ("draw_shim_san" if sanitize else "draw_shim")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else ["-O2"]
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", *flags, "-I", os.path.join(ROOT, "bp_pp_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and sanitize:
        pytest.skip("no sanitizer runtime: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_draw_core_reduction_and_draws_under_gxx(tmp_path, sanitize):
    if sanitize:
        libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
        if not os.path.isabs(libasan) or not os.path.exists(libasan):
            pytest.skip("libasan not present")
    exe = _build_shim(tmp_path, sanitize)
    xs = _chosen_inputs()
    paths = [_fold_trace(x) for x in xs]
    assert {"keep", "sub", "wrap"} <= set(paths), "the chosen inputs must take every final path"
    draws = [(SEED, 0, 0), (SEED, 0, 531), (SEED, (1 << 64) - 1, 600), (bytes(32), 0x4A000000, 7), (b"\xff" * 32, (1 << 32) + 1, 52)]
    lines = [f"R {x.to_bytes(64, 'big').hex()}" for x in xs] + [f"D {s.hex()} {st} {j}" for s, st, j in draws]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.split()
    assert len(out) == len(lines)
    for x, got in zip(xs, out):
        assert int(got, 16) == x % N, hex(x)
        assert int(got, 16) == wide_reduce(x.to_bytes(64, "big"))
    for (s, st, j), got in zip(draws, out[len(xs):]):
        assert int(got, 16) == R.draw(s, st, j)
