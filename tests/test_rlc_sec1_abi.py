"""CPU tier of the wire form's RLC mode and single-proof front end: the new entry points are declared in include/bppp.h, in the
regenerated facade/src/ffi.rs, in bp_pp_amd/_capi.py and exported by the library with the twins' argument lists plus a seed; they refuse
bad arguments before they touch a device; and the batch packing helpers of bp_pp_amd/wire.py round-trip.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bp_pp_amd import wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RLC = ["bppp_%s_verify_batch_rlc_sec1%s" % (v, d) for v in ("u64", "reciprocal", "circuit", "wnla") for d in ("", "_device")]
ONE = ["bppp_%s_verify_one_sec1%s" % (v, t) for v in ("u64", "reciprocal") for t in ("", "_transcript")]


def _params(text, name, opener):
    m = re.search(r"\b%s\s*\((.*?)\)\s*%s" % (name, opener), text, flags=re.S)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def test_new_symbols_are_in_the_header_the_facade_and_the_binding():
    from bp_pp_amd import _capi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bppp.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "facade", "src", "ffi.rs")).read()
    assert sorted(_capi.RLC_SEC1_EXPORTS) == sorted(RLC + ONE)
    for name in RLC + ONE:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, ffi), name
        assert name in _capi.EXPORTS, name
    for name in RLC:
        # the arguments of the exact wire-form twin, then the seed; the u64 device form has the reject counter in place of the trace
        twin = _params(header, name.replace("_rlc_sec1", "_sec1"), ";")
        mine = _params(header, name, ";")
        assert mine[-1] == "const uint8_t seed[32]", name
        if name == "bppp_u64_verify_batch_rlc_sec1_device":
            twin.remove("void* d_trace")
        norm = lambda ps: [re.sub(r"\s+", " ", p).replace("commitments33", "commitments").replace("proofs525", "proofs") for p in ps]
        assert norm(mine[:-1]) == norm(twin), (name, mine, twin)
        assert len(_params(ffi, name, "->")) == len(mine), name
    gpu = open(os.path.join(ROOT, "facade", "src", "gpu.rs")).read()
    assert "pub fn verify_rlc_sec1(" in gpu and "pub fn verify_sec1(" in gpu
    assert "bppp_u64_verify_batch_rlc_sec1(" in gpu and "bppp_u64_verify_one_sec1_transcript(" in gpu


def test_library_exports_them_and_refuses_bad_arguments_without_a_device():
    from bp_pp_amd import _build, _capi
    if not os.path.exists(_build.SO):
        pytest.skip("libbppp_hip.so not built yet")
    L = _capi.lib()
    for name in RLC + ONE:
        assert getattr(L, name).restype is C.c_int, name
    E = _capi.ERR_INVALID_ARG
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    seed = bytes(32)
    acc, st = C.c_uint8(9), C.c_int32(9)
    assert L.bppp_u64_verify_batch_rlc_sec1(None, b"x", 1, 1, p, p, p, p, seed) == E
    assert L.bppp_u64_verify_batch_rlc_sec1_device(None, b"x", 1, 1, p, p, p, p, p, seed) == E
    assert L.bppp_reciprocal_verify_batch_rlc_sec1(None, b"x", 1, 1, 16, 16, p, p, 4, 2, 1, p, p, seed) == E
    assert L.bppp_reciprocal_verify_batch_rlc_sec1_device(None, b"x", 1, 1, 16, 16, p, p, 4, 2, 1, p, p, seed) == E
    assert L.bppp_circuit_verify_batch_rlc_sec1(None, None, b"x", 1, 1, p, p, 4, 2, 1, p, p, seed) == E
    assert L.bppp_circuit_verify_batch_rlc_sec1_device(None, None, b"x", 1, 1, p, p, 4, 2, 1, p, p, seed) == E
    assert L.bppp_wnla_verify_batch_rlc_sec1(None, b"x", 1, 1, p, p, p, p, 4, p, p, p, 2, p, 1, p, p, seed) == E
    assert L.bppp_wnla_verify_batch_rlc_sec1_device(None, b"x", 1, 1, p, p, p, p, 4, p, p, p, 2, p, 1, p, p, seed) == E
    assert L.bppp_u64_verify_one_sec1(None, b"x", 1, bytes(33), bytes(525), C.byref(acc), C.byref(st)) == E
    assert L.bppp_u64_verify_one_sec1_transcript(None, bytes(203), bytes(33), bytes(525), C.byref(acc), C.byref(st)) == E
    assert L.bppp_reciprocal_verify_one_sec1(None, b"x", 1, 16, 16, bytes(33), bytes(525), 4, 2, 1, C.byref(acc), C.byref(st)) == E
    assert L.bppp_reciprocal_verify_one_sec1_transcript(None, bytes(203), 16, 16, bytes(33), bytes(525), 4, 2, 1, C.byref(acc), C.byref(st)) == E
    # a label merlin cannot frame is refused before the transcript is built, with or without a device
    assert L.bppp_u64_verify_one_sec1(None, b"x", C.c_size_t(1 << 32), bytes(33), bytes(525), C.byref(acc), C.byref(st)) == E
    assert (acc.value, st.value) == (9, 9)


def test_python_wrappers_check_seed_and_row_lengths():
    from bp_pp_amd import U64RangeProofProtocol
    from bp_pp_amd.wnla import ArithmeticCircuit, ReciprocalRangeProofProtocol, WeightNormLinearArgument
    u = object.__new__(U64RangeProofProtocol)       # (the checks come before anything touches the context)
    with pytest.raises(ValueError):
        u.verify_batch_rlc_sec1(np.zeros((1, 33), np.uint8), np.zeros((1, 525), np.uint8), b"l", bytes(31))
    with pytest.raises(ValueError):
        u.verify_batch_rlc_sec1_device(b"l", 1, 1, 1, 1, bytes(33))
    with pytest.raises(ValueError):
        u.verify_one_sec1(bytes(64), bytes(525), b"l")
    r = object.__new__(ReciprocalRangeProofProtocol)
    with pytest.raises(ValueError):
        r.verify_batch_rlc_sec1(b"l", np.zeros((1, 33), np.uint8), np.zeros((1, 525), np.uint8), 4, 2, 1, bytes(5))
    with pytest.raises(ValueError):
        r.verify_one_sec1(bytes(33), bytes(524), 4, 2, 1, b"l")
    for cls in (ArithmeticCircuit, WeightNormLinearArgument):
        with pytest.raises(ValueError):
            object.__new__(cls).verify_batch_rlc_sec1_device(b"l", *([1] * (8 if cls is ArithmeticCircuit else 14)), b"short")


def _valid_points(count):
    pts, x = [], 1
    while len(pts) < count:
        rhs = (x ** 3 + 7) % wire.P
        y = pow(rhs, (wire.P + 1) // 4, wire.P)
        if y * y % wire.P == rhs:
            pts.append(x.to_bytes(32, "big") + (y if len(pts) % 2 else wire.P - y).to_bytes(32, "big"))
        x += 1
    return pts


def test_expand_and_pack_round_trip():
    pts = _valid_points(7)
    sc = [bytes([i]) * 32 for i in range(1, 4)]
    rows64 = np.frombuffer(b"".join([pts[0] + pts[1] + sc[0], pts[2] + bytes(64) + sc[1], pts[3] + pts[4] + sc[2]]), np.uint8).reshape(3, 160)
    rows33 = wire.pack(rows64, 2, 1)
    assert rows33.shape == (3, 98) and rows33.dtype == np.uint8
    assert bytes(rows33[0]) == wire.compress_point(pts[0]) + wire.compress_point(pts[1]) + sc[0]
    assert bytes(rows33[1][33:66]) == bytes(33)                                      # the identity: 33 zero bytes
    assert (wire.expand(rows33, 2, 1) == rows64).all()
    assert (wire.expand(rows33.tobytes(), 2, 1) == rows64).all()                     # bytes in, as well as arrays
    assert (wire.pack(wire.expand(rows33, 2, 1), 2, 1) == rows33).all()
    u64 = np.frombuffer(b"".join(pts[i % 7] for i in range(13)) + b"".join(sc), np.uint8).reshape(1, 928)
    assert bytes(wire.pack(u64, 13, 3)[0]) == wire.abi_to_sec1(u64.tobytes())
    with pytest.raises(ValueError):
        wire.expand(bytes(97), 2, 1)
    with pytest.raises(ValueError):
        wire.pack(bytes(161), 2, 1)
    assert wire.expand(b"", 2, 1).shape == (0, 160) and wire.pack(b"", 2, 1).shape == (0, 98)


def test_expand_maps_undecodable_points_to_the_off_curve_point_and_never_to_the_identity():
    good = wire.compress_point(_valid_points(1)[0])
    nonres = next(x for x in range(2, 100) if pow((x ** 3 + 7) % wire.P, (wire.P - 1) // 2, wire.P) == wire.P - 1)
    bad = [b"\x04" + good[1:], b"\x00" + good[1:], b"\x02" + wire.P.to_bytes(32, "big"), b"\x03" + (2 ** 256 - 1).to_bytes(32, "big"),
           b"\x02" + bytes(32), b"\x03" + bytes(32), b"\x02" + nonres.to_bytes(32, "big"), b"\x00" + bytes(31) + b"\x01"]
    assert wire.OFF_CURVE_XY64 == bytes(31) + b"\x01" + bytes(32)
    for enc in bad:
        assert not wire.decodable(enc) and wire.expand_point(enc) == wire.OFF_CURVE_XY64, enc.hex()
        row = wire.expand(good + enc + bytes(32), 2, 1)[0].tobytes()
        assert row == wire.decompress_point(good) + wire.OFF_CURVE_XY64 + bytes(32)
    assert wire.decodable(bytes(33)) and wire.expand_point(bytes(33)) == bytes(64)
    assert wire.decodable(good) and wire.expand_point(good) == wire.decompress_point(good)
    x, y = 1, 0
    assert (y * y - x ** 3 - 7) % wire.P != 0                                        # (1, 0) is not on the curve
