"""The random-linear-combination (RLC) batch mode over the WIRE form (include/bppp.h: bppp_u64_verify_batch_rlc_sec1[_device] and
bppp_{reciprocal,circuit,wnla}_verify_batch_rlc_sec1[_device]) on the GPU.  Three-way agreement, host and device forms: accept bits
and statuses equal (1) the 64-byte RLC call on `wire.expand(...)` of the same bytes with the same seed, (2) the exact wire-form call,
(3) the oracle's verdict on the expanded bytes.  Proofs come from the oracle's provers (tests/workload.py, tests/generic_batches.py and
the case modules) and are packed with bp_pp_amd/wire.py.

An undecodable point -- a bad tag, x = p, `02 || 0`, an x whose x^3 + 7 is a non-residue -- flags its own instance
BPPP_ST_BAD_ENCODING and nobody else: every case below puts such an instance into a chunk (and a superchunk) with valid ones.

Sizes.  u64: n = 64 + 8 + 3 with "rlc_superchunk" = 64 and "rlc_chunk" = 8 (otherwise chosen from the previous call's reject rate):
one complete superchunk through the bucket stage, one complete chunk of 8, a ragged tail.  Generic verifiers: n = 7 (no complete chunk),
8 and 19 (two chunks and a tail).  The rule "fewer than 8 instances run the exact final sum and report last_rlc_chunk = 0" is the WNLA
and circuit verifiers' (include/bppp.h); the reciprocal RLC verifier runs its chunk stage at every n, so for it the wire form is held
to what its 64-byte twin reports."""
import numpy as np
import pytest

import generic_batches as GB
from bp_pp_amd import wire

pytestmark = pytest.mark.gpu

SEED_A, SEED_B = bytes(range(11, 43)), bytes(range(90, 122))
BAD_ENCODING = 1
SUPER, CHUNK = 64, 8
N_U64 = SUPER + CHUNK + 3
U64_POINTS, U64_SCALARS = 13, 3


def _need_gpu():
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")


def _nonresidue_x() -> int:
    x = 2
    while pow((x ** 3 + 7) % wire.P, (wire.P - 1) // 2, wire.P) != wire.P - 1:
        x += 1
    return x


def undecodable_encodings(valid33: bytes):
    """name -> 33 bytes k256's from_bytes refuses"""
    return {"bad tag": b"\x05" + valid33[1:], "x = p": b"\x02" + wire.P.to_bytes(32, "big"), "02 || 0": b"\x02" + bytes(32),
            "non-residue x": b"\x03" + _nonresidue_x().to_bytes(32, "big")}


def u8(blob: bytes) -> np.ndarray:
    return np.frombuffer(blob, np.uint8)


def dev(a: np.ndarray):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------- u64
@pytest.fixture(scope="module")
def u64():
    """The context, the oracle's 75 proofs in the wire form, and the generators."""
    _need_gpu()
    import workload
    from bp_pp_amd import U64RangeProofProtocol
    gens, V, P, _ = workload.make_batch(N_U64, first=8800)
    g, gv, hv = workload.split_generators(gens)
    p = U64RangeProofProtocol(g, gv, hv, device=0, fb_window_bits=8)
    p.set_option("rlc_superchunk", SUPER)
    p.set_option("rlc_chunk", CHUNK)
    yield p, gens, wire.pack(V, 1), wire.pack(P, U64_POINTS, U64_SCALARS)
    p.close()


def _u64_cases(V33, P33):
    """name -> (V33, P33, indices of the invalid proofs, indices of the undecodable ones)"""
    cases = {}
    cases["a: all valid"] = (V33.copy(), P33.copy(), [], [])
    v, p = V33.copy(), P33.copy()
    for i in (10, N_U64 - 2):                                  # the superchunk, the ragged tail
        p[i, 33 * U64_POINTS + 40] ^= 4                        # a proof scalar, below its top byte: well-encoded, wrong
    cases["b: invalid in the superchunk and in the tail"] = (v, p, [10, N_U64 - 2], [])
    v, p = V33.copy(), P33.copy()
    enc = undecodable_encodings(bytes(P33[0, :33]))
    p[5, 0:33] = u8(enc["bad tag"])                            # c_l of proof 5 (superchunk, chunk 0)
    v[20] = u8(enc["x = p"])                                   # the commitment of proof 20 (superchunk, chunk 2)
    p[SUPER + 2, 33 * 12:33 * 13] = u8(enc["02 || 0"])         # the reciprocal r of proof 66 (the complete chunk of 8)
    p[N_U64 - 1, 33 * 8:33 * 9] = u8(enc["non-residue x"])     # x[0] of the last proof (the tail)
    v[33] = 0                                                  # 33 zero bytes: the identity as a commitment -- decodable, and wrong
    cases["c: every undecodable form, and an identity commitment"] = (v, p, [33], [5, 20, SUPER + 2, N_U64 - 1])
    v, p = V33.copy(), P33.copy()
    for i in range(SUPER, SUPER + CHUNK):
        p[i, 33 * U64_POINTS + 70] ^= 1
    cases["d: a whole chunk of 8 invalid"] = (v, p, list(range(SUPER, SUPER + CHUNK)), [])
    return cases


def _u64_device(p, label, V, P, seed, sec1):
    import torch
    n = V.shape[0]
    dV, dP = dev(V), dev(P)
    dA = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    dS = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    dR = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    call = p.verify_batch_rlc_sec1_device if sec1 else p.verify_batch_rlc_device
    call(label, n, dV.data_ptr(), dP.data_ptr(), dA.data_ptr(), seed, d_status=dS.data_ptr(), d_reject_count=dR.data_ptr())
    p.synchronize()
    torch.cuda.synchronize()
    return dA.cpu().numpy(), dS.cpu().numpy(), int(dR.cpu().numpy()[0])


@pytest.mark.parametrize("name", ["a: all valid", "b: invalid in the superchunk and in the tail",
                                  "c: every undecodable form, and an identity commitment", "d: a whole chunk of 8 invalid"])
def test_u64_rlc_sec1_equals_64_byte_rlc_exact_sec1_and_oracle(u64, oracle_c, name):
    import workload
    p, gens, V33, P33 = u64
    v33, p33, invalid, undecodable = _u64_cases(V33, P33)[name]
    v64, p64 = wire.expand(v33, 1), wire.expand(p33, U64_POINTS, U64_SCALARS)
    label = workload.LABEL
    # the oracle on every row of the expanded batch (75 rows: the sample the check asks for, and the rest)
    o_acc, o_st = oracle_c.u64_verify_batch(gens, label, v64, p64, nthreads=4)
    bad = sorted(invalid + undecodable)
    assert [i for i in range(N_U64) if not o_acc[i]] == bad, name
    assert [i for i in range(N_U64) if o_st[i]] == undecodable, name

    acc_x, st_x = p.verify_batch_sec1(v33, p33, label)                       # the exact wire form
    for seed in (SEED_A, SEED_B):
        acc_t, st_t = p.verify_batch_rlc(v64, p64, label, seed)              # the 64-byte RLC twin on the expanded bytes
        used = (p.get_option("last_rlc_superchunk"), p.get_option("last_rlc_chunk"))
        acc, st = p.verify_batch_rlc_sec1(v33, p33, label, seed)
        assert (p.get_option("last_rlc_superchunk"), p.get_option("last_rlc_chunk")) == used == (SUPER, CHUNK), name
        print(name, "rejected", np.flatnonzero(acc == 0).tolist(), "flagged", np.flatnonzero(st).tolist())
        assert acc.tobytes() == acc_t.tobytes() and st.tobytes() == st_t.tobytes(), (name, "vs the 64-byte RLC twin")
        assert acc.tobytes() == acc_x.tobytes() and st.tobytes() == st_x.tobytes(), (name, "vs the exact wire form")
        assert (acc == o_acc).all() and ((st != 0) == (o_st != 0)).all(), (name, "vs the oracle")
        assert all(st[i] == BAD_ENCODING and not acc[i] for i in undecodable), name
        # the device forms, and their reject counters
        acc_dt, st_dt, rej_t = _u64_device(p, label, v64, p64, seed, sec1=False)
        acc_d, st_d, rej = _u64_device(p, label, v33, p33, seed, sec1=True)
        assert acc_d.tobytes() == acc_dt.tobytes() == acc.tobytes() and st_d.tobytes() == st_dt.tobytes() == st.tobytes(), (name, "device")
        assert rej == rej_t == int((acc_d == 0).sum()) == len(bad), (name, rej, rej_t)


def test_u64_rlc_sec1_reject_rate_feeds_the_next_plan(u64):
    """"rlc_reject_ppm" after a wire-form call is what the 64-byte call leaves: the rate of the call just made."""
    import workload
    p, gens, V33, P33 = u64
    v33, p33, invalid, undecodable = _u64_cases(V33, P33)["d: a whole chunk of 8 invalid"]
    p.set_option("rlc_history", 0)
    assert p.get_option("rlc_has_history") == 0
    p.verify_batch_rlc_sec1(v33, p33, workload.LABEL, SEED_A)
    assert p.get_option("rlc_has_history") == 1
    assert p.get_option("rlc_reject_ppm") == int(CHUNK / N_U64 * 1e6 + 0.5)      # 8 of 75, in parts per million


def test_u64_rlc_sec1_allocation_failures_are_nomem_and_the_context_recovers(u64):
    """inject_alloc_fault = k for k = 1, 2, ... on a fresh context each: the k-th device allocation of the host form fails, the call
    returns BPPP_ERR_NOMEM and the same context then serves it.  At least five sites: the four and more of the 64-byte RLC host path
    (I/O staging, per-proof workspace, window tables, RLC buffers, ...) and the buffer the wire form is expanded into."""
    import workload
    from bp_pp_amd._capi import ERR_NOMEM, BpppError
    p, gens, V33, P33 = u64
    v33, p33, invalid, undecodable = _u64_cases(V33, P33)["c: every undecodable form, and an identity commitment"]
    want_acc, want_st = p.verify_batch_sec1(v33, p33, workload.LABEL)
    walked = 0
    for k in range(1, 16):
        c = p.clone_shared()
        try:
            c.set_option("rlc_superchunk", SUPER)
            c.set_option("inject_alloc_fault", k)
            try:
                acc, st = c.verify_batch_rlc_sec1(v33, p33, workload.LABEL, SEED_A)
                reached = False
            except BpppError as e:
                assert e.code == ERR_NOMEM, (k, e.code, str(e))
                reached = True
                acc, st = c.verify_batch_rlc_sec1(v33, p33, workload.LABEL, SEED_A)       # the next call succeeds
            c.set_option("inject_alloc_fault", 0)
            assert acc.tobytes() == want_acc.tobytes() and st.tobytes() == want_st.tobytes(), k
        finally:
            c.close()
        if not reached:
            break
        walked += 1
    assert 5 <= walked < 15, walked


def test_u64_rlc_sec1_edge_arguments(u64):
    import workload
    from bp_pp_amd import _capi
    p, gens, V33, P33 = u64
    L = _capi.lib()
    acc, st = np.full(8, 9, np.uint8), np.full(8, 9, np.int32)
    args = (p._ctx, workload.LABEL, len(workload.LABEL), 8, V33.ctypes.data, P33.ctypes.data, acc.ctypes.data, st.ctypes.data)
    assert L.bppp_u64_verify_batch_rlc_sec1(*args, None) == _capi.ERR_INVALID_ARG                          # no seed
    assert L.bppp_u64_verify_batch_rlc_sec1_device(*args, None, None) == _capi.ERR_INVALID_ARG
    assert L.bppp_u64_verify_batch_rlc_sec1(None, *args[1:], SEED_A) == _capi.ERR_INVALID_ARG              # no context
    assert L.bppp_u64_verify_batch_rlc_sec1(*args[:4], None, *args[5:], SEED_A) == _capi.ERR_INVALID_ARG   # no commitments
    assert acc.tolist() == [9] * 8
    assert L.bppp_u64_verify_batch_rlc_sec1(*args[:3], 0, *args[4:], SEED_A) == _capi.OK                   # an empty batch
    assert L.bppp_u64_verify_batch_rlc_sec1(*args, SEED_A) == _capi.OK and acc.all() and not st.any()


def test_reciprocal_16_16_rlc_sec1_on_a_u64_shaped_context_takes_the_u64_path(oracle_c):
    """dim_nd = dim_np = 16 over 16 + 32 generators with the standard proof shape is the u64 protocol: the wire-form RLC call runs the
    u64 verifier ("last_verify_plan" is set, "last_generic_form" is not), as its exact twin does."""
    _need_gpu()
    import workload
    from bp_pp_amd.wnla import ReciprocalRangeProofProtocol
    n = 19
    gens, V, P, _ = workload.make_batch(n, first=8900)
    P = P.copy()
    P[4, 900] ^= 2
    v33, p33 = wire.pack(V, 1), wire.pack(P, U64_POINTS, U64_SCALARS)
    p33[13, 33:66] = u8(b"\x02" + bytes(32))
    v64, p64 = wire.expand(v33, 1), wire.expand(p33, U64_POINTS, U64_SCALARS)
    o_acc, o_st = oracle_c.u64_verify_batch(gens, workload.LABEL, v64, p64, nthreads=4)
    g, gv, hv = workload.split_generators(gens)
    r = ReciprocalRangeProofProtocol(16, 16, g, gv, hv[:26], [], hv[26:], device=0, fb_window_bits=8)
    try:
        assert r.get_option("last_verify_plan") == 0
        acc, st = r.verify_batch_rlc_sec1(workload.LABEL, v33, p33, 4, 2, 1, SEED_A)
        assert r.get_option("last_verify_plan") != 0 and r.get_option("last_generic_form") == 0
        assert r.get_option("last_rlc_chunk") in (8, 32)
        acc_t, st_t = r.verify_batch_rlc(workload.LABEL, v64, p64, 4, 2, 1, SEED_A)
        acc_x, st_x = r.verify_batch_sec1(workload.LABEL, v33, p33, 4, 2, 1)
        assert acc.tobytes() == acc_t.tobytes() == acc_x.tobytes() and st.tobytes() == st_t.tobytes() == st_x.tobytes()
        assert (acc == o_acc).all() and ((st != 0) == (o_st != 0)).all()
        assert [i for i in range(n) if not acc[i]] == [4, 13] and st[13] == BAD_ENCODING and st[4] == 0
        import torch
        dV, dP = dev(v33), dev(p33)
        dA, dS = torch.full((n,), 9, dtype=torch.uint8, device="cuda"), torch.full((n,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.verify_batch_rlc_sec1_device(workload.LABEL, n, dV.data_ptr(), dP.data_ptr(), 4, 2, 1, dA.data_ptr(), dS.data_ptr(), SEED_B)
        r.synchronize()
        assert dA.cpu().numpy().tobytes() == acc.tobytes() and dS.cpu().numpy().tobytes() == st.tobytes()
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------------------- generic verifiers
KINDS = ("recip8x4", "recip32x16", "mixed_k2", "ac_works", "wnla3x5", "wnla16x32")
SIZES = (7, 8, 19)
SMALL = 8                                  # oracle instances of the shapes that have no pool in tests/generic_batches.py
WNLA_KEYS = ("commitments", "c", "rho", "mu", "proof_r", "proof_x", "proof_l", "proof_n")
_sources = {}


def _protocol(kind):
    return "wnla" if kind.startswith("wnla") else "recip" if kind.startswith("recip") else "circuit"


def _source(kind):
    """The oracle instances of a shape, every one accepted by the oracle (the pools of tests/generic_batches.py where they fit)."""
    if kind in _sources:
        return _sources[kind]
    import circuit_cases
    import recip_cases
    import wnla_cases
    pools = {"wnla16x32": "wnla", "mixed_k2": "circuit", "recip32x16": "recip"}
    if kind in pools:
        case = GB.pool(pools[kind])
    else:
        import bppp_oracle_c as OC
        OC.build()
        if kind == "ac_works":
            case = circuit_cases.make("ac_works", SMALL)
            ok = [circuit_cases.oracle_verify(case, case["commitments"][i].tobytes(), case["proofs"][i].tobytes()) for i in range(SMALL)]
        elif kind == "recip8x4":
            case = recip_cases.make(8, 4, SMALL)
            ok = [recip_cases.oracle_verify(case, case["commitments"][i].tobytes(), case["proofs"][i].tobytes()) for i in range(SMALL)]
        else:
            case = wnla_cases.make(3, 5, SMALL)
            ok = [wnla_cases.oracle_verify(case, i) for i in range(SMALL)]
        assert ok == [1] * SMALL, (kind, ok)
    _sources[kind] = case
    return case


def _shape(kind):
    case = _source(kind)
    return (case["rounds"], case["pl"], case["pn"]) if _protocol(kind) == "circuit" else (case["rounds"], case["nl"], case["nn"])


def _head_points(kind):
    return {"recip": 5, "circuit": 4}[_protocol(kind)]


def _batch(kind, n):
    """n instances in the 64-byte form (tests/generic_batches.py's layout); for n = 19 instance 3 is invalid (a proof scalar changed)."""
    case, protocol = _source(kind), _protocol(kind)
    idx = np.arange(n) % case["commitments"].shape[0]
    if protocol == "wnla":
        b = {k: case[k] for k in ("g", "gv", "hv", "ng", "nh", "label")}
        for k in WNLA_KEYS:
            b[k] = np.ascontiguousarray(case[k][idx])
    else:
        b = {"commitments": np.ascontiguousarray(case["commitments"][idx]), "proofs": np.ascontiguousarray(case["proofs"][idx])}
    b.update(case=case, n=n, protocol=protocol, kind=kind)
    if n == 19:
        GB._scalar_slot(protocol, b, 3, 0)[17] ^= 0x10
    return b


def _to_wire(kind, b):
    """The batch packed into the wire form; for n = 19 round point x[0] of instance 12 (another chunk than instance 3's) is `02 || 0`."""
    rounds, nl, nn = _shape(kind)
    n = b["n"]
    w = dict(b)
    if b["protocol"] == "wnla":
        w["commitments"] = wire.pack(b["commitments"], 1)
        w["proof_r"] = wire.pack(b["proof_r"].reshape(n, -1), rounds).reshape(n, rounds, 33)
        w["proof_x"] = wire.pack(b["proof_x"].reshape(n, -1), rounds).reshape(n, rounds, 33)
        if n == 19:
            w["proof_x"][12, 0] = u8(b"\x02" + bytes(32))
    else:
        k = b["case"]["k"] if b["protocol"] == "circuit" else 1
        P = _head_points(kind) + 2 * rounds
        w["commitments"] = wire.pack(b["commitments"].reshape(n, -1), k)
        w["proofs"] = wire.pack(b["proofs"], P, nl + nn)
        if n == 19:
            o = 33 * (4 + rounds)
            w["proofs"][12, o:o + 33] = u8(b"\x02" + bytes(32))
    return w


def _expanded(kind, w):
    """wire.expand of the wire batch: what the device makes of it, in the 64-byte layout"""
    rounds, nl, nn = _shape(kind)
    n = w["n"]
    e = dict(w)
    if w["protocol"] == "wnla":
        e["commitments"] = wire.expand(w["commitments"], 1)
        e["proof_r"] = wire.expand(w["proof_r"].reshape(n, -1), rounds).reshape(n, rounds, 64)
        e["proof_x"] = wire.expand(w["proof_x"].reshape(n, -1), rounds).reshape(n, rounds, 64)
    else:
        k = w["case"]["k"] if w["protocol"] == "circuit" else 1
        e["commitments"] = wire.expand(w["commitments"], k).reshape(n, -1) if k == 1 else wire.expand(w["commitments"], k).reshape(n, k, 64)
        e["proofs"] = wire.expand(w["proofs"], _head_points(kind) + 2 * rounds, nl + nn)
    return e


def _oracle(kind, e):
    """The oracle on every instance of the expanded batch -> (accept [n], flagged [n])"""
    import recip_cases
    protocol, case = _protocol(kind), e["case"]
    if protocol == "recip":
        rcs = GB._oracle_map(lambda i: recip_cases.oracle_verify(case, e["commitments"][i].tobytes(), e["proofs"][i].tobytes()), range(e["n"]))
    else:
        rcs = GB._oracle_map(lambda i: GB._oracle_rc(protocol, e, i), range(e["n"]))
    return np.array([1 if rc == 1 else 0 for rc in rcs], np.uint8), np.array([rc < 0 for rc in rcs])


def _make_verifier(kind):
    from bp_pp_amd.wnla import ArithmeticCircuit, ReciprocalRangeProofProtocol, WeightNormLinearArgument
    case, protocol = _source(kind), _protocol(kind)
    if protocol == "wnla":
        return WeightNormLinearArgument(case["g"], case["gv"], case["hv"], device=0, fb_window_bits=8)
    if protocol == "recip":
        return ReciprocalRangeProofProtocol(case["nd"], case["np"], case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0,
                                            fb_window_bits=8)
    part = lambda typ, j: (None if case["part"][typ][j] < 0 else int(case["part"][typ][j]))
    arr = lambda blob: np.frombuffer(blob, np.uint8).reshape(-1, 32)
    return ArithmeticCircuit(case["nm"], case["no"], case["k"], case["nv"], case["g"], case["gv"], case["hv"], arr(case["Wm_bytes"]),
                             arr(case["Wl_bytes"]), arr(case["am_bytes"]), arr(case["al_bytes"]), case["f_l"], case["f_m"], case["gv_"],
                             case["hv_"], part, device=0, fb_window_bits=8)


def _host(v, kind, b, mode, seed=None):
    """mode: "rlc64" (the 64-byte RLC twin), "sec1" (the exact wire form), "rlc_sec1" """
    label = b["case"]["label"]
    fn = {"rlc64": v.verify_batch_rlc, "sec1": v.verify_batch_sec1, "rlc_sec1": v.verify_batch_rlc_sec1}[mode]
    tail = () if mode == "sec1" else (seed,)
    if b["protocol"] == "wnla":
        return fn(label, *(b[k] for k in WNLA_KEYS), *tail)
    return fn(label, b["commitments"], b["proofs"], *_shape(kind), *tail)


def _device(v, kind, w, seed):
    """the wire-form RLC device entry point over torch tensors; an instance no kernel reached keeps accept 9 / status 7"""
    import torch
    n, label = w["n"], w["case"]["label"]
    keys = WNLA_KEYS if w["protocol"] == "wnla" else ("commitments", "proofs")
    d = {k: dev(w[k]) for k in keys}
    dA = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    dS = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rounds, nl, nn = _shape(kind)
    if w["protocol"] == "wnla":
        v.verify_batch_rlc_sec1_device(label, n, d["commitments"].data_ptr(), d["c"].data_ptr(), d["rho"].data_ptr(), d["mu"].data_ptr(),
                                       rounds, d["proof_r"].data_ptr(), d["proof_x"].data_ptr(), d["proof_l"].data_ptr(), nl,
                                       d["proof_n"].data_ptr(), nn, dA.data_ptr(), dS.data_ptr(), seed)
    else:
        v.verify_batch_rlc_sec1_device(label, n, d["commitments"].data_ptr(), d["proofs"].data_ptr(), rounds, nl, nn, dA.data_ptr(),
                                       dS.data_ptr(), seed)
    v.synchronize()
    torch.cuda.synchronize()
    return dA.cpu().numpy(), dS.cpu().numpy()


@pytest.fixture(scope="module")
def verifiers():
    _need_gpu()
    made = {}
    try:
        for kind in KINDS:
            made[kind] = _make_verifier(kind)
        yield made
    finally:
        for v in made.values():
            v.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_generic_rlc_sec1_equals_64_byte_rlc_exact_sec1_and_oracle(verifiers, kind, n):
    v = verifiers[kind]
    rounds, nl, nn = _shape(kind)
    assert rounds > 0, kind                                          # (the undecodable point below is a round point)
    w = _to_wire(kind, _batch(kind, n))
    e = _expanded(kind, w)
    o_acc, o_flag = _oracle(kind, e)                                 # every instance
    bad = [3, 12] if n == 19 else []
    assert [i for i in range(n) if not o_acc[i]] == bad and [i for i in range(n) if o_flag[i]] == bad[1:], (kind, n)

    acc_x, st_x = _host(v, kind, w, "sec1")
    acc_t, st_t = _host(v, kind, e, "rlc64", SEED_A)
    used = (v.get_option("last_rlc_superchunk"), v.get_option("last_rlc_chunk"))
    if _protocol(kind) != "recip":                                   # the WNLA / circuit rule (include/bppp.h)
        assert used[1] == (0 if n < CHUNK else CHUNK), (kind, n, used)
    acc, st = _host(v, kind, w, "rlc_sec1", SEED_A)
    assert (v.get_option("last_rlc_superchunk"), v.get_option("last_rlc_chunk")) == used, (kind, n)
    print(kind, n, "rejected", np.flatnonzero(acc == 0).tolist(), "flagged", np.flatnonzero(st).tolist(), "superchunk, chunk", used)
    assert acc.tobytes() == acc_t.tobytes() and st.tobytes() == st_t.tobytes(), (kind, n, "vs the 64-byte RLC twin")
    assert acc.tobytes() == acc_x.tobytes() and st.tobytes() == st_x.tobytes(), (kind, n, "vs the exact wire form")
    assert (acc == o_acc).all() and ((st != 0) == o_flag).all(), (kind, n, "vs the oracle")
    if n == 19:
        assert st[12] == BAD_ENCODING and st[3] == 0
    acc_d, st_d = _device(v, kind, w, SEED_B)
    assert acc_d.tobytes() == acc.tobytes() and st_d.tobytes() == st.tobytes(), (kind, n, "device form", acc_d.tolist(), st_d.tolist())
    assert (v.get_option("last_rlc_superchunk"), v.get_option("last_rlc_chunk")) == used, (kind, n)


def test_generic_rlc_sec1_edge_arguments(verifiers):
    """A NULL seed is BPPP_ERR_INVALID_ARG, an empty batch BPPP_OK, as for the 64-byte RLC forms."""
    from bp_pp_amd import _capi
    L = _capi.lib()
    acc, st = np.zeros(8, np.uint8), np.zeros(8, np.int32)
    kind = "wnla3x5"
    w = _to_wire(kind, _batch(kind, 8))
    rounds, nl, nn = _shape(kind)
    label = w["case"]["label"]
    p = {k: np.ascontiguousarray(w[k]) for k in WNLA_KEYS}
    wargs = (verifiers[kind]._ctx, label, len(label), 8, p["commitments"].ctypes.data, p["c"].ctypes.data, p["rho"].ctypes.data,
             p["mu"].ctypes.data, rounds, p["proof_r"].ctypes.data, p["proof_x"].ctypes.data, p["proof_l"].ctypes.data, nl,
             p["proof_n"].ctypes.data, nn, acc.ctypes.data, st.ctypes.data)
    assert L.bppp_wnla_verify_batch_rlc_sec1(*wargs, None) == _capi.ERR_INVALID_ARG
    assert L.bppp_wnla_verify_batch_rlc_sec1_device(*wargs, None) == _capi.ERR_INVALID_ARG
    assert L.bppp_wnla_verify_batch_rlc_sec1(*wargs[:3], 0, *wargs[4:], SEED_A) == _capi.OK
    assert L.bppp_wnla_verify_batch_rlc_sec1(*wargs, SEED_A) == _capi.OK and acc.all() and not st.any()
    for kind in ("ac_works", "recip8x4"):
        w = _to_wire(kind, _batch(kind, 8))
        rounds, nl, nn = _shape(kind)
        label = w["case"]["label"]
        v = verifiers[kind]
        com, pr = np.ascontiguousarray(w["commitments"]), np.ascontiguousarray(w["proofs"])
        acc[:] = 0
        if kind == "ac_works":
            args = (v._w._ctx, v._circuit, label, len(label), 8, com.ctypes.data, pr.ctypes.data, rounds, nl, nn, acc.ctypes.data, st.ctypes.data)
            host, device, n_at = L.bppp_circuit_verify_batch_rlc_sec1, L.bppp_circuit_verify_batch_rlc_sec1_device, 4
        else:
            args = (v._w._ctx, label, len(label), 8, v.dim_nd, v.dim_np, com.ctypes.data, pr.ctypes.data, rounds, nl, nn, acc.ctypes.data,
                    st.ctypes.data)
            host, device, n_at = L.bppp_reciprocal_verify_batch_rlc_sec1, L.bppp_reciprocal_verify_batch_rlc_sec1_device, 3
        assert host(*args, None) == _capi.ERR_INVALID_ARG and device(*args, None) == _capi.ERR_INVALID_ARG
        assert host(*args[:n_at], 0, *args[n_at + 1:], SEED_A) == _capi.OK
        assert host(*args, SEED_A) == _capi.OK and acc.all() and not st.any(), kind
