"""The mixed-value-count aggregate PROVER at the ABI level, without a device: the four entry points and the argument check are
declared in include/bppp.h, listed in bp_pp_amd/_capi.py, bound in facade/src/ffi.rs, named in INTEGRATION.md and exported by the built
library; their argument lists are the uniform prover's with k -> (k_max, ks); and every refusal is exercised at its edge.  Without a
device there is no context, so the refusals are asked of bppp_reciprocal_agg_prove_mixed_check_args -- the function the entry points
decide by, on the sizes of the (16, 16, 16) context (256 | 32 generators) -- and of the entry points with a NULL context.  The same
refusals on a live context are in tests/test_gpu_agg_prove_mixed.py."""
import os
import re

import numpy as np

from test_agg_transcript_abi import _header, _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"bppp_reciprocal_agg_prove_values_batch_mixed": "bppp_reciprocal_agg_prove_values_batch",
         "bppp_reciprocal_agg_prove_values_batch_mixed_seeded": "bppp_reciprocal_agg_prove_values_batch_seeded",
         "bppp_reciprocal_agg_prove_values_batch_mixed_device": "bppp_reciprocal_agg_prove_values_batch_device",
         "bppp_reciprocal_agg_prove_values_batch_mixed_seeded_device": "bppp_reciprocal_agg_prove_values_batch_seeded_device"}
NAMES = ["bppp_reciprocal_agg_prove_mixed_check_args"] + list(CALLS)


def test_the_names_in_the_header_the_mirror_the_facade_the_guide_and_the_library():
    from bp_pp_amd import _capi
    assert sorted(NAMES) == sorted(_capi.AGG_MIXED_PROVE_EXPORTS)
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
        assert "`%s`" % name in guide, name
    assert "bppp_reciprocal_agg_prove_values_batch_mixed(" in gpu      # the facade method calls it
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol as P
    for method in ("prove_values_batch_mixed", "prove_values_batch_mixed_seeded", "prove_values_batch_mixed_device",
                   "prove_values_batch_mixed_seeded_device"):
        assert callable(getattr(P, method)), method


def test_argument_lists_are_the_uniform_provers_with_k_max_and_ks():
    header = _header()
    for name, uniform in CALLS.items():
        new, old = _params(header, name), _params(header, uniform)
        i = [n for _, n in old].index("k")
        ks = ("constvoid*", "d_ks") if name.endswith("_device") else ("constuint8_t*", "ks")
        assert new == old[:i] + [("size_t", "k_max"), ks] + old[i + 1:], (name, new)
    assert [n for _, n in _params(header, NAMES[0])] == ["ng", "nh", "n", "k_max", "ks", "ks_on_device", "dim_nd", "dim_np"]


def test_the_header_says_what_the_mixed_prover_is_and_what_is_not_built():
    flat = " ".join(re.sub(r"[/*]", " ", _header()).split())
    assert "a mixed prover, is further below: bppp_reciprocal_agg_prove_values_batch_mixed" in flat
    assert "nothing is forwarded inside a mixed call, as in the mixed verifier" in flat          # k_max = 1
    assert ("NOT built for the mixed prover: the caller-transcript form, the SEC1 output form, sharded groups and the single-proof "
            "front end") in flat


def test_every_refusal_at_its_edge():
    from bp_pp_amd import _capi
    L, E = _capi.lib(), _capi.ERR_INVALID_ARG
    NG, NH = 256, 32

    def check(k_max, nd, np_, ks, dev=0, n=None, ng=NG, nh=NH):
        arr = None if ks is None else np.asarray(ks, np.uint8)
        return L.bppp_reciprocal_agg_prove_mixed_check_args(ng, nh, len(ks) if n is None else n, k_max, None if arr is None else arr.ctypes.data,
                                                            dev, nd, np_)

    ok = [1, 16, 9]
    assert check(16, 16, 16, ok) == 0 and check(16, 16, 16, ok, dev=1) == 0
    for dev in (0, 1):
        assert check(16, 16, 16, None, dev=dev, n=3) == E and check(16, 16, 16, None, dev=dev, n=0) == E      # ks NULL, whatever n
        assert check(0, 16, 16, ok, dev=dev) == E and check(65, 1, 1, ok, dev=dev) == E                       # 1 <= k_max <= 64
        assert check(16, 17, 16, ok, dev=dev) == E and check(64, 5, 4, ok, dev=dev) == E                      # k_max dim_nd <= |g_vec|
        assert check(2, 23, 16, [1], dev=dev) == E                                                            # dim_nd + 10 <= |h_vec|
        assert check(16, 16, 18, ok, dev=dev) == E and check(16, 0, 1, ok, dev=dev) == E and check(16, 16, 0, ok, dev=dev) == E
        # dim_np^dim_nd <= n (x must determine its digits): 16^64 = 2^256 is above the group order, 16^63 is not
        assert check(2, 64, 16, [1], dev=dev, ng=4096, nh=128) == E and check(2, 63, 16, [1], dev=dev, ng=4096, nh=128) == 0
    # the host forms read ks: every 1 <= ks[i] <= k_max, first, middle and last
    for bad in ([0, 16, 9], [1, 0, 9], [1, 16, 0], [17, 1, 1], [1, 17, 1], [1, 1, 17], [255]):
        assert check(16, 16, 16, bad) == E, bad
        assert check(16, 16, 16, bad, dev=1) == 0, bad       # (device memory: not read; the instance is flagged where it is)
    assert check(64, 4, 4, [64, 1]) == 0 and check(64, 4, 4, [65]) == E and check(1, 16, 16, [1]) == 0 and check(1, 16, 16, [2]) == E
    # ... and the edges themselves pass, with n = 0 as with instances
    for n in (None, 0):
        assert check(64, 4, 5, [64], n=n) == 0 and check(11, 22, 23, [11], n=n) == 0 and check(16, 16, 17, [16], n=n) == 0
    assert check(16, 16, 16, [0, 17], n=0) == 0              # (n = 0: nothing of ks is read)


def test_a_null_context_or_a_null_buffer_is_invalid_arg():
    from bp_pp_amd import _capi
    L, E = _capi.lib(), _capi.ERR_INVALID_ARG
    buf = np.ones(1 << 12, np.uint8)
    p = buf.ctypes.data
    seed = bytes(32)
    for n in (0, 1):
        assert L.bppp_reciprocal_agg_prove_values_batch_mixed(None, b"x", 1, n, 2, p, 4, 4, p, p, p, p, p, p) == E
        assert L.bppp_reciprocal_agg_prove_values_batch_mixed_seeded(None, b"x", 1, n, 2, p, 4, 4, p, p, seed, 0, p, p, p) == E
        assert L.bppp_reciprocal_agg_prove_values_batch_mixed_device(None, b"x", 1, n, 2, p, 4, 4, p, p, p, p, p, None) == E
        assert L.bppp_reciprocal_agg_prove_values_batch_mixed_seeded_device(None, b"x", 1, n, 2, p, 4, 4, p, p, seed, 0, p, p, None) == E
        # (a NULL rnd or seed is refused in front of the context check: the buffers are looked at first)
        assert L.bppp_reciprocal_agg_prove_values_batch_mixed(None, b"x", 1, n, 2, p, 4, 4, p, p, None, p, p, p) == E
        assert L.bppp_reciprocal_agg_prove_values_batch_mixed_seeded_device(None, b"x", 1, n, 2, p, 4, 4, p, p, None, 0, p, p, None) == E
