"""CPU tier of the generic proofs' wire form: bp_pp_amd/wire.py's generic SEC1 helpers (round trips at several shapes, identity points in
every position, JSON -> SEC1 -> ABI -> SEC1 -> JSON), the new C entry points' argument checks without a GPU, and the device lane
functions of csrc/wire_core.h compiled for the host against wire.py on OpenSSL's known answers."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from bp_pp_amd import wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "openssl_secp256k1.json")


def _points():
    with open(GOLD) as f:
        return [bytes.fromhex(v["xy"]) for v in json.load(f)["mul_g"]]


def _proof64(n_points, n_scalars, seed, identity_at=()):
    pts = _points()
    out = [bytes(64) if i in identity_at else pts[(seed + 3 * i) % len(pts)] for i in range(n_points)]
    sc = [((seed * 7919 + i) * 0x9E3779B97F4A7C15 % (2 ** 255)).to_bytes(32, "big") for i in range(n_scalars)]
    return b"".join(out) + b"".join(sc)


@pytest.mark.parametrize("kind,rounds,nl,nn", [("reciprocal", 4, 2, 1), ("reciprocal", 8, 3, 2), ("reciprocal", 0, 5, 0),
                                               ("circuit", 3, 2, 2), ("circuit", 1, 1, 1), ("wnla", 2, 0, 0), ("wnla", 0, 0, 0)])
def test_generic_round_trip_with_identity_in_every_position(kind, rounds, nl, nn):
    P = wire.proof_points(kind, rounds)
    S = 0 if kind == "wnla" else nl + nn
    assert wire.abi_proof_bytes(kind, rounds, nl, nn) == 64 * P + 32 * S
    assert wire.sec1_proof_bytes(kind, rounds, nl, nn) == 33 * P + 32 * S
    for hole in [None] + list(range(P)):
        abi = _proof64(P, S, seed=P + (hole or 0), identity_at=() if hole is None else (hole,))
        s1 = wire.generic_abi_to_sec1(abi, P)
        assert len(s1) == wire.sec1_proof_bytes(kind, rounds, nl, nn)
        if hole is not None:
            assert s1[33 * hole:33 * hole + 33] == bytes(33)
        assert s1[33 * P:] == abi[64 * P:]
        assert wire.generic_sec1_to_abi(s1, P, S) == abi


def test_u64_shape_is_the_existing_525_byte_form():
    abi = _proof64(13, 3, seed=5, identity_at=(7,))
    assert wire.generic_abi_to_sec1(abi, 13) == wire.abi_to_sec1(abi)
    assert wire.generic_sec1_to_abi(wire.abi_to_sec1(abi), 13, 3) == abi == wire.sec1_to_abi(wire.abi_to_sec1(abi))


@pytest.mark.parametrize("reciprocal,rounds,nl,nn", [(True, 4, 2, 1), (True, 8, 3, 2), (False, 2, 2, 3), (False, 0, 4, 1)])
def test_json_sec1_abi_cycle(reciprocal, rounds, nl, nn):
    kind = "reciprocal" if reciprocal else "circuit"
    P = wire.proof_points(kind, rounds)
    abi = _proof64(P, nl + nn, seed=11, identity_at=(1, P - 1))
    text = json.dumps(wire.circuit_proof_to_doc(abi, rounds, nl, nn, reciprocal))
    s1 = wire.json_to_generic_sec1(text)
    assert wire.generic_abi_to_sec1(wire.generic_sec1_to_abi(s1, P, nl + nn), P) == s1
    assert json.loads(wire.generic_sec1_to_json(s1, rounds, nl, nn, reciprocal)) == json.loads(text)
    assert wire.doc_to_sec1_proof(wire.sec1_proof_to_doc(s1, rounds, nl, nn, reciprocal)) == s1
    doc = json.loads(text)
    assert (doc["circuit_proof"] if reciprocal else doc)["c_r"] == "00"          # serde's identity


def test_wnla_json_cycle():
    r64, x64 = _proof64(3, 0, seed=2, identity_at=(0,)), _proof64(3, 0, seed=9, identity_at=(2,))
    l, n = _proof64(0, 2, seed=4), _proof64(0, 1, seed=6)
    r33, x33 = wire.generic_abi_to_sec1(r64, 3), wire.generic_abi_to_sec1(x64, 3)
    doc = wire.wnla_sec1_to_doc(r33, x33, l, n)
    assert doc == wire.wnla_proof_to_doc(r64, x64, l, n)
    assert wire.doc_to_wnla_sec1(json.loads(json.dumps(doc))) == (r33, x33, l, n)


def test_undecodable_points_are_refused_on_the_host():
    good = wire.compress_point(_points()[0])
    for bad in (b"\x04" + good[1:], b"\x02" + wire.P.to_bytes(32, "big"), b"\x00" + good[1:]):
        with pytest.raises(ValueError):
            wire.generic_sec1_to_abi(bad + bytes(32), 1, 1)
    with pytest.raises(ValueError):
        wire.generic_sec1_to_abi(good, 1, 1)                                   # wrong length
    with pytest.raises(ValueError):
        wire.proof_points("u64", 4)


NEW = ["bppp_reciprocal_verify_batch_sec1", "bppp_reciprocal_verify_batch_sec1_device", "bppp_circuit_verify_batch_sec1",
       "bppp_circuit_verify_batch_sec1_device", "bppp_wnla_verify_batch_sec1", "bppp_wnla_verify_batch_sec1_device",
       "bppp_reciprocal_prove_batch_sec1", "bppp_circuit_prove_batch_sec1", "bppp_wnla_prove_batch_sec1"]


def test_new_entry_points_are_declared_and_bound():
    from bp_pp_amd import _capi
    text = open(os.path.join(ROOT, "include", "bppp.h")).read()
    for name in NEW:
        assert name in _capi.EXPORTS and f"{name}(" in text


def test_new_entry_points_refuse_a_null_context_without_a_gpu():
    """Every SEC1 entry point of the generic protocols checks its arguments before it touches a device: a NULL context (what a caller
    holds after context creation failed for want of a GPU) is BPPP_ERR_INVALID_ARG, never a crash."""
    from bp_pp_amd import _build, _capi
    if not os.path.exists(_build.SO):
        pytest.fail("libbppp_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    L = _capi.lib()
    E = _capi.ERR_INVALID_ARG
    buf = np.zeros(1 << 16, np.uint8)
    p = buf.ctypes.data
    assert L.bppp_reciprocal_verify_batch_sec1(None, b"x", 1, 1, 32, 16, p, p, 5, 4, 3, p, p) == E
    assert L.bppp_reciprocal_verify_batch_sec1_device(None, b"x", 1, 1, 32, 16, p, p, 5, 4, 3, p, p) == E
    assert L.bppp_circuit_verify_batch_sec1(None, None, b"x", 1, 1, p, p, 2, 2, 1, p, p) == E
    assert L.bppp_circuit_verify_batch_sec1_device(None, None, b"x", 1, 1, p, p, 2, 2, 1, p, p) == E
    assert L.bppp_wnla_verify_batch_sec1(None, b"x", 1, 1, p, p, p, p, 1, p, p, p, 2, p, 2, p, p) == E
    assert L.bppp_wnla_verify_batch_sec1_device(None, b"x", 1, 1, p, p, p, p, 1, p, p, p, 2, p, 2, p, p) == E
    assert L.bppp_reciprocal_prove_batch_sec1(None, b"x", 1, 1, 32, 16, p, p, p, p, p, p, p, p) == E
    assert L.bppp_circuit_prove_batch_sec1(None, None, b"x", 1, 1, p, p, p, p, p, p, p, p, p) == E
    assert L.bppp_wnla_prove_batch_sec1(None, b"x", 1, 1, p, p, p, p, p, 2, p, 2, p, p, p, p, p) == E


HOST_TU = r'''
#include <cstring>
#include "plan_core.h"      // (first: field.h pulls <stdio.h> in inside its namespace in the host build)
#include "wire_core.h"
using namespace bppp;
// n instances of P points + S scalars, contiguous on both sides, every lane of the flat map run in a loop
extern "C" int wire_host(int expand, size_t n, size_t P, size_t S, const uint8_t* src, uint8_t* dst, const int32_t* zero_if) {
    const size_t b33 = 33 * P + 32 * S, b64 = 64 * P + 32 * S;
    WireMap m;
    wire_map_init(m, n);
    m.zero_if = zero_if;
    if (expand) {
        wire_map_add(m, true, src + 33 * P, b33, dst + 64 * P, b64, S);      // (scalars first: finish puts the points in front)
        wire_map_add(m, false, src, b33, dst, b64, P);
    } else {
        wire_map_add(m, true, src + 64 * P, b64, dst + 33 * P, b33, S);
        wire_map_add(m, false, src, b64, dst, b33, P);
    }
    const u64 lanes = wire_map_finish(m);
    if (m.seg[0].scalar && P) return -1;
    for (u64 g = 0; g < lanes; g++) {
        if (expand) wire_expand_lane(m, g);
        else wire_compress_lane(m, g);
    }
    return (int)lanes;
}
'''


@pytest.fixture(scope="module")
def host_wire(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.fail("g++ is needed for the host build of csrc/wire_core.h")
    d = tmp_path_factory.mktemp("wire_host")
    src, so = d / "wire_host.cpp", d / "wire_host.so"
    src.write_text(HOST_TU)
    subprocess.check_call([gxx, "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "bp_pp_amd", "csrc"), "-o", str(so), str(src)])
    L = C.CDLL(str(so))
    L.wire_host.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def test_device_lane_functions_on_the_host_match_wire_py(host_wire):
    pts = _points()
    n, P, S = 7, 5, 3
    b64, b33 = 64 * P + 32 * S, 33 * P + 32 * S
    abi = b"".join(_proof64(P, S, seed=t, identity_at=(t % P,)) for t in range(n))
    s1 = b"".join(wire.generic_abi_to_sec1(abi[i:i + b64], P) for i in range(0, len(abi), b64))
    out33 = np.zeros(len(s1), np.uint8)
    src = np.frombuffer(abi, np.uint8).copy()
    assert host_wire.wire_host(0, n, P, S, src.ctypes.data, out33.ctypes.data, None) == n * (P + 8 * S)
    assert out33.tobytes() == s1
    out64 = np.zeros(len(abi), np.uint8)
    src33 = np.frombuffer(s1, np.uint8).copy()
    host_wire.wire_host(1, n, P, S, src33.ctypes.data, out64.ctypes.data, None)
    assert out64.tobytes() == abi
    # OpenSSL's k*G in its SEC1 form decodes to its affine form, one lane per point
    with open(GOLD) as f:
        sec1 = np.frombuffer(b"".join(bytes.fromhex(v["sec1"]) for v in json.load(f)["mul_g"]), np.uint8).copy()
    out = np.zeros(64 * len(pts), np.uint8)
    host_wire.wire_host(1, len(pts), 1, 0, sec1.ctypes.data, out.ctypes.data, None)
    assert out.tobytes() == b"".join(pts)
    # zero_if: a flagged instance comes out as zero bytes
    flags = np.array([0, 2, 0, 0, 0, 0, 1], np.int32)
    out33[:] = 0xAA
    host_wire.wire_host(0, n, P, S, src.ctypes.data, out33.ctypes.data, flags.ctypes.data)
    for t in range(n):
        assert out33[t * b33:(t + 1) * b33].tobytes() == (bytes(b33) if flags[t] else s1[t * b33:(t + 1) * b33])


def test_undecodable_points_expand_to_the_off_curve_sentinel_on_the_host(host_wire):
    good = wire.compress_point(_points()[3])
    x = 1
    while pow((x ** 3 + 7) % wire.P, (wire.P - 1) // 2, wire.P) != wire.P - 1:
        x += 1
    off, ident = bytes(31) + b"\x01" + bytes(32), bytes(64)
    cases = [(b"\x04" + good[1:], off), (b"\x01" + good[1:], off), (b"\x02" + wire.P.to_bytes(32, "big"), off),
             (b"\x03" + (2 ** 256 - 1).to_bytes(32, "big"), off), (b"\x02" + x.to_bytes(32, "big"), off), (bytes(33), ident),
             (b"\x02" + bytes(32), off), (good, wire.decompress_point(good))]
    src = np.frombuffer(b"".join(c for c, _ in cases), np.uint8).copy()
    out = np.zeros(64 * len(cases), np.uint8)
    host_wire.wire_host(1, len(cases), 1, 0, src.ctypes.data, out.ctypes.data, None)
    assert [out[64 * i:64 * i + 64].tobytes() for i in range(len(cases))] == [e for _, e in cases]
