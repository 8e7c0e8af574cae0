"""The mixed-value-count aggregate's wire (SEC1) form and RLC mode at the ABI level, without a device: the six entry points are
declared in include/bppp.h, listed in bp_pp_amd/_capi.py, bound in facade/src/ffi.rs and exported by the built library; a NULL context
(and, for the RLC forms, a NULL seed) answers BPPP_ERR_INVALID_ARG; and the slot sizes the Python binding lays its buffers out by are
what wire.pack makes of a row for every value count.  The checks on a live context are in tests/test_gpu_agg_mixed_sec1.py and
tests/test_gpu_agg_mixed_rlc.py."""
import os
import re

import numpy as np

import agg_cases as A
from bp_pp_amd import wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOST = ["bppp_reciprocal_agg_verify_batch_mixed_rlc", "bppp_reciprocal_agg_verify_batch_mixed_sec1",
        "bppp_reciprocal_agg_verify_batch_mixed_rlc_sec1"]
DEVICE = [name + "_device" for name in HOST]
NAMES = HOST + DEVICE
SEED = bytes(range(32))


def _lib():
    from bp_pp_amd import _capi
    return _capi.lib(), _capi.ERR_INVALID_ARG


def test_the_six_names_in_the_header_the_mirror_the_facade_and_the_library():
    from bp_pp_amd import _capi
    assert len(set(NAMES)) == 6
    with open(os.path.join(ROOT, "include", "bppp.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "facade", "src", "ffi.rs")) as f:
        ffi = f.read()
    L = _capi.lib()
    for name in NAMES:
        assert re.search(r"BPPP_API\s+int\s+%s\(" % name, header), name
        assert name in _capi.EXPORTS, name
        assert re.search(r"pub fn %s\(" % name, ffi), name
        assert hasattr(L, name), name
    assert "NOT built: the SEC1 form, the RLC form" not in header


def _args(name, ctx, seed):
    """(3, 4, 4)-shaped arguments over buffers no check reads: k_max and ks where the mixed call has them, d_reject_count in front of
    the seed, the seed last."""
    buf = np.ones(1 << 12, np.uint8)
    p = buf.ctypes.data
    args = [ctx, b"x", 1, 1, 3, p, 4, 4, p, p, 4, 2, 1, p, p]
    if name.endswith("_device"):
        args.append(None)
    if "_rlc" in name:
        args.append(seed)
    return buf, args


def test_a_null_context_is_invalid_arg():
    L, E = _lib()
    for name in NAMES:
        buf, args = _args(name, None, SEED)
        assert getattr(L, name)(*args) == E, name


def test_a_null_seed_is_invalid_arg():
    L, E = _lib()
    rlc = [name for name in NAMES if "_rlc" in name]
    assert len(rlc) == 4
    for name in rlc:
        buf, args = _args(name, None, None)
        assert getattr(L, name)(*args) == E, name


def test_slot_sizes_against_wire_pack_for_every_value_count():
    """S(k) = bppp_reciprocal_agg_proof_sec1_bytes(k, rounds, nl, nn) is the length of wire.pack of a k-value proof, never more than the
    slot S(k_max), and l | n sit at 33 (4 + 2 rounds + k); commitments: k x 33 of k_max x 33."""
    L, _ = _lib()
    S = L.bppp_reciprocal_agg_proof_sec1_bytes
    B = L.bppp_reciprocal_agg_proof_bytes
    for k_max, rounds, nl, nn in ((3, 4, 2, 1), (7, 5, 1, 2), (6, 4, 1, 1), (16, 6, 1, 4)):
        slot = S(k_max, rounds, nl, nn)
        for k in range(1, k_max + 1):
            P = 4 + 2 * rounds + k
            row = np.zeros((1, A.proof_bytes(k, rounds, nl, nn)), np.uint8)
            row[0, 64 * P:] = np.arange(32 * (nl + nn)) % 251 + 1
            packed = wire.pack(row, P, nl + nn)
            assert packed.shape[1] == S(k, rounds, nl, nn) == 33 * P + 32 * (nl + nn) <= slot
            assert row.shape[1] == B(k, rounds, nl, nn)
            assert packed[0, 33 * P:].tobytes() == row[0, 64 * P:].tobytes()
            assert wire.pack(np.zeros((1, 64 * k), np.uint8), k).shape[1] == 33 * k <= 33 * k_max
        assert slot - S(k_max - 1, rounds, nl, nn) == 33
