"""CPU tier for the RLC mode of the WNLA and circuit verifiers: the built library exports the four entry points, include/bppp.h
declares them with their exact twins' argument lists plus the seed, without a device they answer as the exact twins do, and the
Python methods refuse a seed that is not 32 bytes before they touch anything else.  The GPU tier is tests/test_gpu_generic_rlc.py."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bppp_wnla_verify_batch_rlc", "bppp_wnla_verify_batch_rlc_device", "bppp_circuit_verify_batch_rlc",
       "bppp_circuit_verify_batch_rlc_device")


def _prototypes():
    """name -> parameter list (comments and whitespace removed) of every BPPP_API declaration of the header."""
    text = open(os.path.join(ROOT, "include", "bppp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, params in re.findall(r"BPPP_API\s+int\s+(bppp_[a-z0-9_]+)\s*\((.*?)\)\s*;", text, flags=re.S):
        out[name] = [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]
    return out


def _lib():
    from bp_pp_amd import _build, _capi
    if not os.path.exists(_build.SO):
        pytest.fail("libbppp_hip.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    return _capi.lib()


def test_header_declares_the_four_with_their_twins_arguments_and_a_seed():
    protos = _prototypes()
    for name in NEW:
        twin = name.replace("_rlc", "")
        assert name in protos and twin in protos, name
        assert protos[name] == protos[twin] + ["const uint8_t seed[32]"], (name, protos[name])


def test_library_exports_the_four_and_the_binding_lists_them():
    from bp_pp_amd import _capi
    L = _lib()
    for name in NEW:
        assert name in _capi.EXPORTS, name
        fn = getattr(L, name, None)
        assert fn is not None, name
        assert fn.restype is _capi.C.c_int and len(fn.argtypes) == len(getattr(L, name.replace("_rlc", "")).argtypes) + 1, name


def test_without_a_context_they_answer_as_the_exact_twins_do():
    """A NULL context -- what a caller is left with where bppp_wnla_ctx_create found no device (BPPP_ERR_NO_DEVICE) -- is
    BPPP_ERR_INVALID_ARG for the exact twins and for the RLC forms alike, with or without a seed: never a crash, never a fallback."""
    import ctypes as C
    import numpy as np
    from bp_pp_amd import _capi
    L = _lib()
    E = _capi.ERR_INVALID_ARG
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    seed = bytes(32)
    wnla = (None, b"x", 1, 1, p, p, p, p, 1, p, p, p, 1, p, 1, p, p)
    circuit = (None, None, b"x", 1, 1, p, p, 1, 1, 1, p, p)
    assert L.bppp_wnla_verify_batch(*wnla) == E and L.bppp_wnla_verify_batch_device(*wnla) == E
    assert L.bppp_circuit_verify_batch(*circuit) == E and L.bppp_circuit_verify_batch_device(*circuit) == E
    for s in (seed, None):
        assert L.bppp_wnla_verify_batch_rlc(*wnla, s) == E
        assert L.bppp_wnla_verify_batch_rlc_device(*wnla, s) == E
        assert L.bppp_circuit_verify_batch_rlc(*circuit, s) == E
        assert L.bppp_circuit_verify_batch_rlc_device(*circuit, s) == E
    import torch
    if torch.cuda.device_count() == 0:
        ctx = C.c_void_p()
        assert L.bppp_wnla_ctx_create(C.byref(ctx), bytes(64), bytes(64), 1, bytes(64), 1, 0, 8) == _capi.ERR_NO_DEVICE and not ctx.value


def test_python_methods_refuse_a_seed_that_is_not_32_bytes():
    """Before anything else: the check needs no context, no circuit and no library."""
    from bp_pp_amd.wnla import ArithmeticCircuit, WeightNormLinearArgument
    w = WeightNormLinearArgument.borrowed(0, 16, 32)
    q = ArithmeticCircuit.__new__(ArithmeticCircuit)
    q._w, q._circuit, q.k = w, None, 1
    for seed in (bytes(31), bytes(33), b""):
        with pytest.raises(ValueError):
            w.verify_batch_rlc(b"x", None, None, None, None, None, None, None, None, seed)
        with pytest.raises(ValueError):
            w.verify_batch_rlc_device(b"x", 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, seed)
        with pytest.raises(ValueError):
            q.verify_batch_rlc(b"x", None, None, 0, 0, 0, seed)
        with pytest.raises(ValueError):
            q.verify_batch_rlc_device(b"x", 1, 0, 0, 0, 0, 0, 0, 0, seed)


def test_a_library_without_the_symbols_is_an_error_not_another_path(monkeypatch):
    """An A/B library of an earlier ABI (BPPP_LIB) lacks the entry points: the methods say so."""
    from bp_pp_amd import _capi, wnla

    class Old:
        pass

    monkeypatch.setattr(_capi, "lib", lambda: Old())
    w = wnla.WeightNormLinearArgument.borrowed(0, 16, 32)
    with pytest.raises(NotImplementedError, match="bppp_wnla_verify_batch_rlc_device"):
        w.verify_batch_rlc_device(b"x", 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, bytes(32))
    with pytest.raises(NotImplementedError, match="bppp_wnla_verify_batch_rlc"):
        w.verify_batch_rlc(b"x", None, None, None, None, None, None, None, None, bytes(32))
