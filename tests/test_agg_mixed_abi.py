"""The mixed-value-count aggregate verifier at the ABI level, without a device: both entry points and the argument check are declared
in include/bppp.h, listed in bp_pp_amd/_capi.py, bound in facade/src/ffi.rs, named in INTEGRATION.md and exported by the built
library; their argument lists are the uniform calls' with k -> (k_max, ks); and every argument check is exercised at its edge.
Without a device there is no context, so the checks are asked of bppp_reciprocal_agg_mixed_check_args -- the function both entry
points take their decision from, on the sizes of the (16, 16, 16) context (256 | 32 generators) -- and of the entry points with a
NULL context.  The same refusals on a live context are in tests/test_gpu_agg_mixed.py."""
import os
import re

import numpy as np

from test_agg_transcript_abi import _header, _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"bppp_reciprocal_agg_verify_batch_mixed": "bppp_reciprocal_agg_verify_batch",
         "bppp_reciprocal_agg_verify_batch_mixed_device": "bppp_reciprocal_agg_verify_batch_device"}
NAMES = ["bppp_reciprocal_agg_mixed_check_args"] + list(CALLS)


def test_the_names_in_the_header_the_mirror_the_facade_the_guide_and_the_library():
    from bp_pp_amd import _capi
    assert sorted(NAMES) == sorted(_capi.AGG_MIXED_EXPORTS)
    header = _header()
    with open(os.path.join(ROOT, "facade", "src", "ffi.rs")) as f:
        ffi = f.read()
    with open(os.path.join(ROOT, "facade", "src", "gpu.rs")) as f:
        gpu = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        guide = f.read()
    L = _capi.lib()
    for name in NAMES:
        assert re.search(r"BPPP_API\s+int\s+%s\(" % name, header), name
        assert name in _capi.EXPORTS, name
        assert re.search(r"pub fn %s\(" % name, ffi), name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == len(_params(header, name)), name
    for name in CALLS:
        assert "`%s`" % name in guide, name
    assert "bppp_reciprocal_agg_verify_batch_mixed(" in gpu      # the facade method calls it


def test_argument_lists_are_the_uniform_calls_with_k_max_and_ks():
    header = _header()
    for name, uniform in CALLS.items():
        new, old = _params(header, name), _params(header, uniform)
        i = [n for _, n in old].index("k")
        ks = ("constvoid*", "d_ks") if name.endswith("_device") else ("constuint8_t*", "ks")
        assert new == old[:i] + [("size_t", "k_max"), ks] + old[i + 1:], (name, new)


def test_the_header_says_what_the_mixed_call_is_and_what_is_not_built():
    flat = " ".join(re.sub(r"[/*]", " ", _header()).split())
    assert "take one k for the whole call; these take one per instance" in flat
    for left_out in ("the SEC1 form, the RLC form and the caller-transcript form of the mixed call", "a mixed prover",
                     "reordering instances by k on the device", "the single-proof front end and sharded groups"):
        assert left_out in flat, left_out


def test_every_argument_check_at_its_edge():
    from bp_pp_amd import _capi
    L, E = _capi.lib(), _capi.ERR_INVALID_ARG
    NG, NH = 256, 32

    def check(k_max, nd, np_, ks, rounds=6, nl=1, nn=4, dev=0, n=None):
        arr = None if ks is None else np.asarray(ks, np.uint8)
        return L.bppp_reciprocal_agg_mixed_check_args(NG, NH, len(ks) if n is None else n, k_max, None if arr is None else arr.ctypes.data, dev,
                                                      nd, np_, rounds, nl, nn)

    ok = [1, 16, 9]
    assert check(16, 16, 16, ok) == 0 and check(16, 16, 16, ok, dev=1) == 0
    for dev in (0, 1):
        assert check(16, 16, 16, None, dev=dev, n=3) == E and check(16, 16, 16, None, dev=dev, n=0) == E      # ks NULL, whatever n
        assert check(0, 16, 16, ok, dev=dev) == E and check(65, 1, 1, ok, dev=dev) == E                       # 1 <= k_max <= 64
        assert check(16, 17, 16, ok, dev=dev) == E and check(64, 5, 4, ok, dev=dev) == E                      # k_max dim_nd <= |g_vec|
        assert check(2, 23, 16, [1], dev=dev) == E                                                            # dim_nd + 10 <= |h_vec|
        assert check(16, 16, 18, ok, dev=dev) == E and check(16, 0, 1, ok, dev=dev) == E and check(16, 16, 0, ok, dev=dev) == E
        assert check(16, 16, 16, ok, rounds=13, dev=dev) == E and check(16, 16, 16, ok, nl=4097, dev=dev) == E
        assert check(16, 16, 16, ok, nn=4097, dev=dev) == E
    # the host form reads ks: every 1 <= ks[i] <= k_max, first, middle and last
    for bad in ([0, 16, 9], [1, 0, 9], [1, 16, 0], [17, 1, 1], [1, 17, 1], [1, 1, 17], [255]):
        assert check(16, 16, 16, bad) == E, bad
        assert check(16, 16, 16, bad, dev=1) == 0, bad       # (device memory: not read; the instance is flagged where it is)
    assert check(64, 4, 4, [64, 1]) == 0 and check(64, 4, 4, [65]) == E and check(1, 16, 16, [1]) == 0 and check(1, 16, 16, [2]) == E
    # ... and the edges themselves pass, with n = 0 as with instances
    for n in (None, 0):
        assert check(64, 4, 5, [64], n=n) == 0 and check(11, 22, 23, [11], n=n) == 0
        assert check(16, 16, 17, [16], rounds=12, nl=4096, nn=4096, n=n) == 0
    assert check(16, 16, 16, [0, 17], n=0) == 0              # (n = 0: nothing of ks is read)


def test_a_null_context_or_a_null_buffer_is_invalid_arg():
    from bp_pp_amd import _capi
    L, E = _capi.lib(), _capi.ERR_INVALID_ARG
    buf = np.ones(1 << 12, np.uint8)
    p = buf.ctypes.data
    for n in (0, 1):
        assert L.bppp_reciprocal_agg_verify_batch_mixed(None, b"x", 1, n, 2, p, 4, 4, p, p, 3, 2, 1, p, p) == E
        assert L.bppp_reciprocal_agg_verify_batch_mixed_device(None, b"x", 1, n, 2, p, 4, 4, p, p, 3, 2, 1, p, p, None) == E
