"""The aggregate's caller-transcript forms at the ABI level, without a device: every new entry point is declared in include/bppp.h,
listed in bp_pp_amd/_capi.py, bound in facade/src/ffi.rs and exported by the built library; its argument list is the label form's
with (label, label_len, n) -> (n, states, n_states) -- the order of every other `_transcript` entry point -- and states_out last; and
the refusals that need no GPU answer BPPP_ERR_INVALID_ARG.  Without a device there is no context, so the refusals here go with a NULL
context or NULL states over buffers that are never read; the same checks on a live context are in tests/test_gpu_agg_transcript.py."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# new name -> the label form whose list it follows
VERIFY = {"bppp_reciprocal_agg_verify_batch_transcript": "bppp_reciprocal_agg_verify_batch",
          "bppp_reciprocal_agg_verify_batch_transcript_device": "bppp_reciprocal_agg_verify_batch_device",
          "bppp_reciprocal_agg_verify_batch_transcript_sec1": "bppp_reciprocal_agg_verify_batch_sec1"}
PROVE = {"bppp_reciprocal_agg_prove_values_batch_transcript": "bppp_reciprocal_agg_prove_values_batch",
         "bppp_reciprocal_agg_prove_values_batch_transcript_seeded": "bppp_reciprocal_agg_prove_values_batch_seeded",
         "bppp_reciprocal_agg_prove_values_batch_transcript_device": "bppp_reciprocal_agg_prove_values_batch_device"}
NAMES = list(VERIFY) + list(PROVE)
SEED = bytes(range(32))


def _header():
    with open(os.path.join(ROOT, "include", "bppp.h")) as f:
        return f.read()


def _params(header, name):
    """[(type, name)] of a prototype of the header, comments dropped."""
    m = re.search(r"BPPP_API\s+int\s+%s\((.*?)\);" % name, header, re.S)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for a in args.split(","):
        a = re.sub(r"\[\d*\]$", "*", " ".join(a.split()))
        mm = re.match(r"(.*?)(\w+)(\*?)$", a)
        out.append((mm.group(1).replace(" ", "") + mm.group(3), mm.group(2)))
    return out


def test_the_six_names_in_the_header_the_mirror_the_facade_and_the_library():
    from bp_pp_amd import _capi
    assert len(NAMES) == len(set(NAMES)) == 6
    assert sorted(NAMES) == sorted(_capi.AGG_TRANSCRIPT_EXPORTS)
    header = _header()
    with open(os.path.join(ROOT, "facade", "src", "ffi.rs")) as f:
        ffi = f.read()
    L = _capi.lib()
    for name in NAMES:
        assert re.search(r"BPPP_API\s+int\s+%s\(" % name, header), name
        assert name in _capi.EXPORTS, name
        assert re.search(r"pub fn %s\(" % name, ffi), name
        assert hasattr(L, name), name
        # bound by lib(): an argument list of the header's length (an unbound ctypes function has none).  The return type cannot be
        # told from ctypes' default, which is the C int these return; _capi sets it all the same.
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == len(_params(header, name)), name


def test_argument_lists_are_the_label_forms_with_the_states_substituted():
    header = _header()
    for name, label_form in list(VERIFY.items()) + list(PROVE.items()):
        new, old = _params(header, name), _params(header, label_form)
        assert [n for _, n in old[:4]] == ["ctx", "label", "label_len", "n"], label_form
        device = name.endswith("_device")
        states = [("constvoid*", "d_states")] if device else [("constuint8_t*", "states")]
        out = ("void*", "d_states_out") if device else ("uint8_t*", "states_out")
        assert new == [old[0], old[3]] + states + [("size_t", "n_states")] + old[4:] + [out], (name, new)


def test_the_header_says_what_is_left_and_that_there_is_no_rlc_form():
    flat = " ".join(re.sub(r"[/*]", " ", _header()).split())
    assert "a caller-transcript form, a sharded form and a single-proof front end are not built" not in flat
    assert "a sharded form and a single-proof front end are not built" in flat
    assert "no RLC transcript form" in flat


def _verify_args(name, ctx, states, n, n_states, k=2):
    buf = np.zeros(1 << 12, np.uint8)
    p = buf.ctypes.data
    args = [ctx, n, p if states else None, n_states, k, 4, 4, p, p, 3, 2, 1, p, p]
    if name.endswith("_device"):
        args.append(None)
    return buf, args + [p]


def _prove_args(name, ctx, states, n, n_states, k=2):
    buf = np.zeros(1 << 12, np.uint8)
    p = buf.ctypes.data
    draws = [SEED, 0] if "seeded" in name else [p]
    return buf, [ctx, n, p if states else None, n_states, k, 4, 4, p, p] + draws + [p, p, p, p]


def _call(L, name, *a, **kw):
    buf, args = (_verify_args if name in VERIFY else _prove_args)(name, *a, **kw)
    return getattr(L, name)(*args)


def test_a_null_context_is_invalid_arg():
    """With n = 0 and with buffers that are never read.  Every other refusal (NULL states, n_states, the k range) is decided against
    a live context, which needs a device: tests/test_gpu_agg_transcript.py::test_argument_refusals."""
    from bp_pp_amd import _capi
    L, E = _capi.lib(), _capi.ERR_INVALID_ARG
    for name in NAMES:
        for n in (0, 1):
            assert _call(L, name, None, True, n, 1) == E, (name, n)
