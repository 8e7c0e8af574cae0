"""The aggregate's wire (SEC1) form and RLC mode at the ABI level, without a device: every new entry point is declared in
include/bppp.h, listed in bp_pp_amd/_capi.py, bound in facade/src/ffi.rs and exported by the built library; the wire proof's size is
what the layout says; and the argument checks that need no GPU -- a NULL context, a NULL seed, a label merlin cannot frame -- answer
BPPP_ERR_INVALID_ARG.  Without a device there is no context, so the seed and label cases here go with a NULL context; the same two
checks on a live context, where nothing else is wrong with the call, are in tests/test_gpu_agg_rlc.py."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZE = "bppp_reciprocal_agg_proof_sec1_bytes"
VERIFY_HOST = ["bppp_reciprocal_agg_verify_batch_sec1", "bppp_reciprocal_agg_verify_batch_rlc", "bppp_reciprocal_agg_verify_batch_rlc_sec1"]
VERIFY_DEVICE = [name + "_device" for name in VERIFY_HOST]
PROVE = ["bppp_reciprocal_agg_prove_values_batch_sec1", "bppp_reciprocal_agg_prove_values_batch_seeded_sec1"]
NAMES = [SIZE] + VERIFY_HOST + VERIFY_DEVICE + PROVE
RLC = [name for name in VERIFY_HOST + VERIFY_DEVICE if "_rlc" in name]
SEED = bytes(range(32))


def _lib():
    from bp_pp_amd import _capi
    return _capi.lib(), _capi.ERR_INVALID_ARG


def test_every_new_name_in_the_header_the_mirror_the_facade_and_the_library():
    from bp_pp_amd import _capi
    assert len(NAMES) == len(set(NAMES)) == 9          # the size, six verifier forms, two prover forms
    with open(os.path.join(ROOT, "include", "bppp.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "facade", "src", "ffi.rs")) as f:
        ffi = f.read()
    L = _capi.lib()
    for name in NAMES:
        assert re.search(r"BPPP_API\s+(int|size_t)\s+%s\(" % name, header), name
        assert name in _capi.EXPORTS, name
        assert re.search(r"pub fn %s\(" % name, ffi), name
        assert hasattr(L, name), name


def test_wire_proof_bytes():
    L, _ = _lib()
    f = getattr(L, SIZE)
    assert f(16, 6, 1, 4) == 1216 == 33 * (4 + 12 + 16) + 32 * 5       # sixteen u64 values
    assert f(1, 4, 2, 1) == 525                                         # k = 1 over the u64 generators: the u64 wire proof
    assert f(2, 3, 2, 1) == 33 * 12 + 32 * 3


def _verify_args(name, ctx, label, label_len, seed):
    """(2, 4, 4)-shaped arguments over buffers no check reads; the device forms take d_reject_count before the seed."""
    buf = np.zeros(1 << 12, np.uint8)
    p = buf.ctypes.data
    args = [ctx, label, label_len, 1, 2, 4, 4, p, p, 3, 2, 1, p, p]
    if name.endswith("_device"):
        args.append(None)
    if "_rlc" in name:
        args.append(seed)
    return buf, args


def _prove_args(name, ctx, label, label_len, seed):
    buf = np.zeros(1 << 12, np.uint8)
    p = buf.ctypes.data
    draws = [seed, 0] if "seeded" in name else [p]
    return buf, [ctx, label, label_len, 1, 2, 4, 4, p, p] + draws + [p, p, p]


def test_a_null_context_is_invalid_arg():
    L, E = _lib()
    for name in VERIFY_HOST + VERIFY_DEVICE:
        buf, args = _verify_args(name, None, b"x", 1, SEED)
        assert getattr(L, name)(*args) == E, name
    for name in PROVE:
        buf, args = _prove_args(name, None, b"x", 1, SEED)
        assert getattr(L, name)(*args) == E, name


def test_a_null_seed_is_invalid_arg():
    L, E = _lib()
    assert len(RLC) == 4
    for name in RLC:
        buf, args = _verify_args(name, None, b"x", 1, None)
        assert getattr(L, name)(*args) == E, name
    buf, args = _prove_args(PROVE[1], None, b"x", 1, None)
    assert getattr(L, PROVE[1])(*args) == E


def test_a_label_merlin_cannot_frame_is_invalid_arg():
    L, E = _lib()
    too_long = C.c_size_t(1 << 32)
    for name in VERIFY_HOST + VERIFY_DEVICE:
        buf, args = _verify_args(name, None, b"x", too_long, SEED)
        assert getattr(L, name)(*args) == E, name
    for name in PROVE:
        buf, args = _prove_args(name, None, b"x", too_long, SEED)
        assert getattr(L, name)(*args) == E, name
