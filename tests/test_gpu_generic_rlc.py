"""The random-linear-combination (RLC) mode of the WNLA and circuit verifiers (bppp_wnla_verify_batch_rlc[_device],
bppp_circuit_verify_batch_rlc[_device]) on the GPU: accept bits and statuses equal the exact entry points' and the oracle's verdicts
at every batch size around the chunk of 8 -- no complete chunk (1, 7: the exact final sum by the stated rule), exactly one (8), one
over (9), two (16), a ragged tail (70) -- and with the bucket stage over superchunks of 64 (2 x 64 + 3 instances: two complete
superchunks and a ragged one) and without it.

Every verdict is the oracle's: the untouched instances are oracle instances the oracle accepted (tests/generic_batches.py: pool();
the small shapes are verified here), and every corrupted instance gets an oracle call of its own.  Batches are those instances
repeated, corrupted with the helpers of tests/generic_batches.py.

Shapes: WNLA over 16 + 32 generators (the u64 size, 4 rounds), the ragged (3, 5) and the (1, 2) shape; circuits `mixed_k2` (k = 2,
all four partition types) and the reference's own `ac_works`."""
import ctypes as C

import numpy as np
import pytest

import generic_batches as GB

pytestmark = pytest.mark.gpu

KINDS = ("wnla16x32", "wnla3x5", "wnla1x2", "mixed_k2", "ac_works")
SIZES = (1, 7, 8, 9, 16, 70)
CHUNK = 8
SUPER = 64                                   # the smallest superchunk "rlc_superchunk" takes
N_SUPER = 2 * SUPER + 3
SEED_A, SEED_B = bytes(range(7, 39)), bytes(range(200, 232))
SMALL = 16                                   # oracle instances of the shapes that have no pool
WNLA_KEYS = ("commitments", "c", "rho", "mu", "proof_r", "proof_x", "proof_l", "proof_n")

_sources = {}


def _protocol(kind):
    return "wnla" if kind.startswith("wnla") else "circuit"


def _source(kind):
    """The oracle instances of a shape, every one accepted by the oracle."""
    if kind in _sources:
        return _sources[kind]
    import circuit_cases
    import wnla_cases
    if kind == "wnla16x32":
        case = GB.pool("wnla")
    elif kind == "mixed_k2":
        case = GB.pool("circuit")
    else:
        import bppp_oracle_c as OC
        OC.build()
        if kind == "ac_works":
            case = circuit_cases.make("ac_works", SMALL)
            ok = [circuit_cases.oracle_verify(case, case["commitments"][i].tobytes(), case["proofs"][i].tobytes()) for i in range(SMALL)]
        else:
            case = wnla_cases.make(*{"wnla3x5": (3, 5), "wnla1x2": (1, 2)}[kind], SMALL)
            ok = [wnla_cases.oracle_verify(case, i) for i in range(SMALL)]
        assert ok == [1] * SMALL, (kind, ok)
    _sources[kind] = case
    return case


def _batch(kind, n):
    """n instances: source instance i mod P at place i, in the form tests/generic_batches.py's helpers take."""
    case, protocol = _source(kind), _protocol(kind)
    idx = np.arange(n) % case["commitments"].shape[0]
    if protocol == "wnla":
        b = {k: case[k] for k in ("g", "gv", "hv", "ng", "nh", "label")}
        for k in WNLA_KEYS:
            b[k] = np.ascontiguousarray(case[k][idx])
    else:
        b = {"commitments": np.ascontiguousarray(case["commitments"][idx]), "proofs": np.ascontiguousarray(case["proofs"][idx])}
    b.update(case=case, n=n, protocol=protocol, kind=kind, bad=[])
    return b


def _tamper(b, i):
    """Well-formed and wrong: a bit flipped in the last proof scalar (never its top byte: the value stays below the group order)."""
    GB._scalar_slot(b["protocol"], b, i, 0)[17] ^= 0x10
    b["bad"].append(i)


def _malform(b, i):
    """A bad encoding: an off-curve round point where the shape has rounds, else a proof scalar equal to the group order."""
    import bppp_oracle as O
    if b["case"]["rounds"] > 0:
        GB._round_point(b["protocol"], b, i, 0)[63] ^= 1
    else:
        GB._scalar_slot(b["protocol"], b, i, 0)[:] = np.frombuffer(O.N.to_bytes(32, "big"), np.uint8)
    b["bad"].append(i)


def _expect(b):
    """The oracle's verdict on all n instances: accept bits, and where it raised an encoding error."""
    acc, flag = np.ones(b["n"], np.uint8), np.zeros(b["n"], bool)
    for i in sorted(set(b["bad"])):
        rc = GB._oracle_rc(b["protocol"], b, i)
        acc[i], flag[i] = (1 if rc == 1 else 0), rc < 0
    return acc, flag


def _shape(b):
    case = b["case"]
    return (case["rounds"], case["pl"], case["pn"]) if b["protocol"] == "circuit" else (case["rounds"], case["nl"], case["nn"])


def _host(v, b, seed=None):
    label = b["case"]["label"]
    if b["protocol"] == "wnla":
        args = {k: b[k] for k in WNLA_KEYS}
        return v.verify_batch(label, **args) if seed is None else v.verify_batch_rlc(label, **args, seed=seed)
    if seed is None:
        return v.verify_batch(label, b["commitments"], b["proofs"], *_shape(b))
    return v.verify_batch_rlc(label, b["commitments"], b["proofs"], *_shape(b), seed=seed)


def _device(v, b, seed=None):
    """The device-resident entry points over torch tensors; an instance no kernel reached keeps accept 9 / status 7."""
    import torch
    n, label = b["n"], b["case"]["label"]
    keys = WNLA_KEYS if b["protocol"] == "wnla" else ("commitments", "proofs")
    d = {k: torch.from_numpy(b[k]).cuda() for k in keys}
    dA = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    dS = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rounds, nl, nn = _shape(b)
    if b["protocol"] == "wnla":
        args = (label, n, d["commitments"].data_ptr(), d["c"].data_ptr(), d["rho"].data_ptr(), d["mu"].data_ptr(), rounds,
                d["proof_r"].data_ptr(), d["proof_x"].data_ptr(), d["proof_l"].data_ptr(), nl, d["proof_n"].data_ptr(), nn, dA.data_ptr(),
                dS.data_ptr())
    else:
        args = (label, n, d["commitments"].data_ptr(), d["proofs"].data_ptr(), rounds, nl, nn, dA.data_ptr(), dS.data_ptr())
    if seed is None:
        v.verify_batch_device(*args)
    else:
        v.verify_batch_rlc_device(*args, seed)
    v.synchronize()
    torch.cuda.synchronize()
    return dA.cpu().numpy(), dS.cpu().numpy()


def _make_verifier(kind, fb_window_bits):
    from bp_pp_amd.wnla import ArithmeticCircuit, WeightNormLinearArgument
    case = _source(kind)
    if _protocol(kind) == "wnla":
        return WeightNormLinearArgument(case["g"], case["gv"], case["hv"], device=0, fb_window_bits=fb_window_bits)
    part = lambda typ, j: (None if case["part"][typ][j] < 0 else int(case["part"][typ][j]))
    arr = lambda blob: np.frombuffer(blob, np.uint8).reshape(-1, 32)
    return ArithmeticCircuit(case["nm"], case["no"], case["k"], case["nv"], case["g"], case["gv"], case["hv"], arr(case["Wm_bytes"]),
                             arr(case["Wl_bytes"]), arr(case["am_bytes"]), arr(case["al_bytes"]), case["f_l"], case["f_m"], case["gv_"],
                             case["hv_"], part, device=0, fb_window_bits=fb_window_bits)


@pytest.fixture(scope="module")
def verifiers():
    """Per shape one context that chooses its superchunk by itself ("auto") and one whose "rlc_superchunk" the tests set ("fixed": the
    option cannot be put back to automatic).  8-bit tables: small and quick to build, the same kernels."""
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    made = {}
    try:
        for kind in KINDS:
            made[(kind, "auto")] = _make_verifier(kind, 8)
            made[(kind, "fixed")] = _make_verifier(kind, 8)
        yield made
    finally:
        for v in made.values():
            v.close()


def _check(v, b, used, what):
    """RLC host form, the exact host form right after it, the RLC host and device forms with another seed: all the oracle's verdicts,
    byte-equal to one another, and the context reports the superchunk / chunk it used."""
    tag = (b["kind"], b["n"], what)
    exp_acc, exp_flag = _expect(b)
    acc_r, st_r = _host(v, b, SEED_A)
    assert (v.get_option("last_rlc_superchunk"), v.get_option("last_rlc_chunk")) == used, tag
    form_r = v.get_option("last_generic_form")
    acc_e, st_e = _host(v, b)                                    # an exact call on the same context right after an RLC call
    assert form_r == v.get_option("last_generic_form") != 0, tag
    assert (acc_e == exp_acc).all() and ((st_e != 0) == exp_flag).all(), (tag, "exact vs oracle", acc_e.tolist(), st_e.tolist(), b["bad"])
    assert acc_r.tobytes() == acc_e.tobytes() and st_r.tobytes() == st_e.tobytes(), (tag, "rlc host", acc_r.tolist(), st_r.tolist(), b["bad"])
    acc_b, st_b = _host(v, b, SEED_B)                            # another seed, the same form
    assert acc_b.tobytes() == acc_r.tobytes() and st_b.tobytes() == st_r.tobytes(), (tag, "rlc host, second seed", acc_b.tolist(), st_b.tolist())
    acc_d, st_d = _device(v, b, SEED_B)                          # that seed, the device form
    assert acc_d.tobytes() == acc_e.tobytes() and st_d.tobytes() == st_e.tobytes(), (tag, "rlc device", acc_d.tolist(), st_d.tolist(), b["bad"])
    assert (v.get_option("last_rlc_superchunk"), v.get_option("last_rlc_chunk")) == used, tag
    return exp_acc, exp_flag


def _contents(kind, n):
    """(name, batch) for every content the size admits."""
    out = []
    b = _batch(kind, n)
    out.append(("all valid", b))
    b = _batch(kind, n)
    for i in range(n):
        _tamper(b, i)
    out.append(("all invalid", b))
    if n >= CHUNK:
        b = _batch(kind, n)
        _tamper(b, 3)
        out.append(("one tampered in a chunk", b))
        b = _batch(kind, n)
        _tamper(b, 3)
        _tamper(b, 5)
        out.append(("two tampered in one chunk", b))
        b = _batch(kind, n)
        _malform(b, 2)
        out.append(("a bad encoding in a chunk", b))
    if n % CHUNK:
        b = _batch(kind, n)
        _tamper(b, n - 1)
        out.append(("tampered in the incomplete last chunk", b))
        b = _batch(kind, n)
        _malform(b, n - 1)
        out.append(("a bad encoding in the incomplete last chunk", b))
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_rlc_equals_exact_and_oracle_around_the_chunk_size(verifiers, kind, n):
    """The automatic superchunk: 256 at these sizes (the smallest the automatic choice takes), i.e. one ragged superchunk in front
    of the chunks of 8.  A call without a complete chunk runs the exact final sum and reports (0, 0)."""
    v = verifiers[(kind, "auto")]
    used = (256, CHUNK) if n >= CHUNK else (0, 0)
    for what, b in _contents(kind, n):
        exp_acc, exp_flag = _check(v, b, used, what)
        bad = sorted(set(b["bad"]))
        assert [i for i in range(n) if not exp_acc[i]] == bad, (kind, n, what)          # the other seven (all others) are accepted
        assert int(exp_flag.sum()) == ("bad encoding" in what), (kind, n, what)


@pytest.mark.parametrize("kind", KINDS)
def test_rlc_bucket_stage_on_two_superchunks_and_a_ragged_one_and_off(verifiers, kind):
    """2 x 64 + 3 instances with "rlc_superchunk" = 64: superchunks that pass on their one combined check, one that falls through to
    the chunks of 8 and the exact sum, and a ragged third; then the same batches with the stage off."""
    v = verifiers[(kind, "fixed")]
    n = N_SUPER
    batches = [("all valid", _batch(kind, n))]
    b = _batch(kind, n)
    _tamper(b, 11)                               # superchunk 0 fails, 1 and 2 pass
    batches.append(("one tampered in superchunk 0", b))
    b = _batch(kind, n)
    _tamper(b, SUPER + 9)
    _tamper(b, SUPER + 14)                       # two of one chunk of superchunk 1
    _malform(b, 20)                              # superchunk 0: a flagged instance has weight zero, the superchunk still passes
    _tamper(b, n - 1)                            # the ragged superchunk, its incomplete chunk
    batches.append(("tampered in superchunks 1 and 2, a bad encoding in 0", b))
    b = _batch(kind, n)
    for i in range(n):
        _tamper(b, i)
    batches.append(("all invalid", b))
    for M in (SUPER, 0):
        v.set_option("rlc_superchunk", M)
        for what, b in batches:
            _check(v, b, (M, CHUNK), (what, M))


@pytest.mark.parametrize("kind", ["wnla16x32", "mixed_k2"])
def test_rlc_kernels_show_in_the_timings(verifiers, kind):
    """With kernel timing on, the chunk stage and the bucket stage in front of it are in bppp_ctx_get_timings, one launch each; the
    exact call of the same batch launches the one final sum it always did."""
    v = verifiers[(kind, "auto")]
    b = _batch(kind, 70)
    _tamper(b, 13)
    _malform(b, 42)
    exp_acc, exp_flag = _expect(b)
    v.enable_timing(True)
    try:
        v.timings()                                  # (reset)
        acc, st = _device(v, b, SEED_A)
        kt = v.timings()
        acc_e, st_e = _device(v, b)
        ke = v.timings()
    finally:
        v.enable_timing(False)
    assert (acc == exp_acc).all() and ((st != 0) == exp_flag).all() and acc.tobytes() == acc_e.tobytes() and st.tobytes() == st_e.tobytes()
    for name in ("k_wnla_rlc_lhs", "k_wnla_rlc_chunk", "k_wnla_rlc_check", "k_bkt_prepare", "k_bkt_accumulate", "k_bkt_scalars", "k_bkt_check"):
        assert kt[name]["launches"] == 1, (name, kt.get(name))
        assert name not in ke or ke[name]["launches"] == 0, (name, ke.get(name))
    assert kt["k_wnla_msm"]["launches"] == 2 and kt["k_wnla_accept"]["launches"] == 1          # the flagged chunks' exact sums: sparse and dense form
    assert ke["k_wnla_msm"]["launches"] == 1 and ke["k_wnla_accept"]["launches"] == 1
    assert kt["k_wnla_round"]["launches"] == ke["k_wnla_round"]["launches"] == b["case"]["rounds"]


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("kind", ["wnla16x32", "mixed_k2"])
def test_rlc_allocation_failures_are_nomem_and_the_context_recovers(kind, form):
    """Every device allocation of an RLC call fails once (inject_alloc_fault = k): BPPP_ERR_NOMEM, and the same context then serves the
    same call.  The batch grows from walk to walk so that every grow-only buffer of the call is allocated anew.  Four sites: the window
    tables' scratch (ensure_straus_capacity), the bucket stage's workspace, the call's blob, the round points' tables."""
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    from bp_pp_amd._capi import ERR_NOMEM, BpppError
    v = _make_verifier(kind, 8)
    run = _host if form == "host" else _device
    try:
        walked = 0
        for k in range(1, 8):
            b = _batch(kind, 6 + 64 * k)
            _tamper(b, 5)
            _malform(b, 64 * k)
            exp_acc, exp_flag = _expect(b)
            v.set_option("inject_alloc_fault", k)
            try:
                acc, st = run(v, b, SEED_A)
                reached = False
            except BpppError as e:
                assert e.code == ERR_NOMEM, (k, e.code, str(e))
                reached = True
                acc, st = run(v, b, SEED_A)                       # the same context serves the call
            v.set_option("inject_alloc_fault", 0)
            assert (acc == exp_acc).all() and ((st != 0) == exp_flag).all(), (kind, form, k)
            if not reached:
                break
            walked += 1
        assert walked == 4, walked
    finally:
        v.close()


def test_rlc_edge_arguments_on_a_live_context(verifiers):
    """A NULL seed is BPPP_ERR_INVALID_ARG whatever else is given; an empty batch is BPPP_OK as for the exact twins."""
    from bp_pp_amd import _capi
    L = _capi.lib()
    w, q = verifiers[("wnla1x2", "auto")], verifiers[("ac_works", "auto")]
    b = _batch("wnla1x2", 8)
    p = {k: b[k].ctypes.data for k in WNLA_KEYS}
    rounds, nl, nn = _shape(b)
    acc, st = np.zeros(8, np.uint8), np.zeros(8, np.int32)
    label = b["case"]["label"]
    wargs = (w._ctx, label, len(label), 8, p["commitments"], p["c"], p["rho"], p["mu"], rounds, p["proof_r"], p["proof_x"], p["proof_l"], nl,
             p["proof_n"], nn, acc.ctypes.data, st.ctypes.data)
    assert L.bppp_wnla_verify_batch_rlc(*wargs, None) == _capi.ERR_INVALID_ARG
    assert L.bppp_wnla_verify_batch_rlc_device(*wargs, None) == _capi.ERR_INVALID_ARG
    assert L.bppp_wnla_verify_batch_rlc(*wargs[:3], 0, *wargs[4:], SEED_A) == _capi.OK == L.bppp_wnla_verify_batch(*wargs[:3], 0, *wargs[4:])
    assert L.bppp_wnla_verify_batch_rlc(*wargs, SEED_A) == _capi.OK and acc.all() and not st.any()
    c = _batch("ac_works", 8)
    rounds, nl, nn = _shape(c)
    label = c["case"]["label"]
    cargs = (q._w._ctx, q._circuit, label, len(label), 8, c["commitments"].ctypes.data, c["proofs"].ctypes.data, rounds, nl, nn,
             acc.ctypes.data, st.ctypes.data)
    acc[:] = 0
    assert L.bppp_circuit_verify_batch_rlc(*cargs, None) == _capi.ERR_INVALID_ARG
    assert L.bppp_circuit_verify_batch_rlc_device(*cargs, None) == _capi.ERR_INVALID_ARG
    assert L.bppp_circuit_verify_batch_rlc(*cargs[:4], 0, *cargs[5:], SEED_A) == _capi.OK == L.bppp_circuit_verify_batch(*cargs[:4], 0, *cargs[5:])
    assert L.bppp_circuit_verify_batch_rlc(*cargs, SEED_A) == _capi.OK and acc.all() and not st.any()
