"""Large batches for the generic verifiers (WeightNormLinearArgument, ArithmeticCircuit, ReciprocalRangeProofProtocol) whose EVERY
verdict is the oracle's.  The oracle's provers make one instance in tens of milliseconds, so a batch of n is a pool of P = 257 distinct
oracle instances repeated: instance i is pool entry i mod 257 (257 is prime, hence coprime to the block size and to every lane-group
size: each lane position meets every pool entry).  The batch is then corrupted at the places a wrong grid or a wrong lane group would
lose -- block edges, the last wavefront of every lane-group size, the last instance -- and each corrupted instance gets its expectation
from an oracle call of its own; every other instance expects accept = 1, status = 0 because its pool entry verified under the oracle.
The expectation covers all n instances; nothing is sampled.

    build(protocol, n) -> dict: the entry point's arrays, "expect_acc" [n] uint8, "expect_flag" [n] bool, "bad" (corrupted indices),
                                "case" (generators and shape, as the case module made them)
protocol: "wnla" (16 + 32 generators, 4 rounds), "circuit" (`mixed_k2`, 2 rounds), "recip" (dim_nd = 32, dim_np = 16, 5 rounds)."""
import ctypes as C
import hashlib
import os
import pickle

import numpy as np

import bppp_oracle as O

POOL = 257
PROTOCOLS = ("wnla", "circuit", "recip")
BUILDERS = {"wnla": ("wnla_cases", (16, 32, POOL)), "circuit": ("circuit_cases", ("mixed_k2", POOL)), "recip": ("recip_cases", (32, 16, POOL))}
GROUP_SIZES = (2, 4, 8, 16)
FIELD_P = 2**256 - 2**32 - 977
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CACHE_DIR = os.path.join(ROOT, "build", "generic_pool")          # git-ignored

_pools = {}


def _cases(protocol):
    import importlib
    return importlib.import_module(BUILDERS[protocol][0])


def _cache_path(protocol):
    """Keyed by the builder's arguments and by the text of what builds the instances (the case module and the oracle)."""
    mod, args = BUILDERS[protocol]
    h = hashlib.sha256()
    for path in (os.path.join(ROOT, "tests", mod + ".py"), os.path.join(ROOT, "oracle", "bppp_ref.c")):
        with open(path, "rb") as f:
            h.update(f.read())
    return os.path.join(CACHE_DIR, "%s-%s-%s.pkl" % (mod, "-".join(str(a) for a in args), h.hexdigest()[:16]))


def _oracle_map(fn, items):
    """Independent oracle calls on a few threads (ctypes drops the GIL for the call; the oracle keeps no state between calls)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as ex:
        return list(ex.map(fn, items))


def pool_verdicts(protocol, case):
    """The oracle's verdict on every pool entry (1 = accept)."""
    cases = _cases(protocol)
    if protocol == "wnla":
        return _oracle_map(lambda b: cases.oracle_verify(case, b), range(POOL))
    return _oracle_map(lambda b: cases.oracle_verify(case, case["commitments"][b].tobytes(), case["proofs"][b].tobytes()), range(POOL))


def pool(protocol):
    """The 257 oracle instances of a protocol, each accepted by the oracle: cached per process, and as a pickle under build/ (the
    provers take the better part of a minute for the three pools)."""
    if protocol in _pools:
        return _pools[protocol]
    import bppp_oracle_c as OC
    OC.build()
    path = _cache_path(protocol)
    case = None
    if os.path.exists(path):
        try:
            with open(path, "rb") as f:
                case = pickle.load(f)
        except Exception:
            case = None
    if case is None:
        mod, args = BUILDERS[protocol]
        case = _cases(protocol).make(*args)
        assert pool_verdicts(protocol, case) == [1] * POOL, protocol
        try:
            os.makedirs(CACHE_DIR, exist_ok=True)
            with open(path + ".tmp%d" % os.getpid(), "wb") as f:
                pickle.dump({k: v for k, v in case.items() if k != "dims"}, f)          # (dims: a ctypes array, rebuilt below)
            os.replace(path + ".tmp%d" % os.getpid(), path)
        except OSError:
            pass                                                                        # a read-only tree: no cache, same pool
    if protocol == "circuit" and "dims" not in case:
        case["dims"] = (C.c_size_t * 6)(case["nm"], case["no"], case["k"], case["nl"], case["nv"], case["nw"])
    _pools[protocol] = case
    return case


def last_wavefront_first(n, group):
    """With `group` lanes per instance a wavefront of 64 lanes holds 64 / group instances: the first instance of the batch's last
    (possibly ragged) wavefront; its last one is n - 1."""
    per = 64 // group
    return (n - 1) // per * per


def tamper_positions(n, rng):
    fixed = [0, 63, 64, n - 2, n - 1] + [last_wavefront_first(n, g) for g in GROUP_SIZES]
    rand = [int(i) for i in rng.integers(0, n, 24)]
    return sorted(set(i for i in fixed + rand if 0 <= i < n))


# ---- per protocol: where a proof scalar, a round point and the commitment of instance i live in the batch's arrays
def _scalar_slot(protocol, b, i, j):
    """A writable view of 32 bytes: proof scalar j of instance i, counted from the end of the proof (n, then l)."""
    if protocol == "wnla":
        nn = b["proof_n"].shape[1]
        return b["proof_n"][i, j] if j < nn else b["proof_l"][i, j - nn]
    P = b["proofs"]
    return P[i, P.shape[1] - 32 * (j + 1):P.shape[1] - 32 * j]


def _round_point(protocol, b, i, k):
    """A writable view of the 64 bytes of round point x[k] of instance i."""
    if protocol == "wnla":
        return b["proof_x"][i, k]
    o = 256 + 64 * b["case"]["rounds"] + 64 * k          # circuit and reciprocal proofs alike: 256 bytes of points, r[rounds], x[rounds]
    return b["proofs"][i, o:o + 64]


def _n_scalars(protocol, b):
    case = b["case"]
    return case["pl"] + case["pn"] if protocol == "circuit" else case["nl"] + case["nn"]


def _oracle_rc(protocol, b, i):
    cases = _cases(protocol)
    if protocol == "wnla":
        return cases.oracle_verify(b, i)
    return cases.oracle_verify(b["case"], b["commitments"][i].tobytes(), b["proofs"][i].tobytes())


def build(protocol, n):
    """The corrupted batch of n instances and the oracle's verdict on all of them; deterministic in (protocol, n)."""
    assert protocol in PROTOCOLS and n >= 130
    case = pool(protocol)
    idx = np.arange(n) % POOL
    if protocol == "wnla":
        b = {k: case[k] for k in ("g", "gv", "hv", "ng", "nh", "label")}
        for k in ("commitments", "c", "rho", "mu", "proof_r", "proof_x", "proof_l", "proof_n"):
            b[k] = np.ascontiguousarray(case[k][idx])
    else:
        b = {"commitments": np.ascontiguousarray(case["commitments"][idx]), "proofs": np.ascontiguousarray(case["proofs"][idx])}
    b["case"], b["n"], b["protocol"] = case, n, protocol
    rng = np.random.default_rng([PROTOCOLS.index(protocol), n])
    # tampered, well-formed: a bit flipped in a proof scalar (never its top byte: the value stays below the group order), or the
    # commitment of another pool entry
    tampered = tamper_positions(n, rng)
    for i in tampered:
        if rng.integers(0, 3) == 0:
            b["commitments"][i] = case["commitments"][(i + 1 + int(rng.integers(0, POOL - 1))) % POOL]
        else:
            slot = _scalar_slot(protocol, b, i, int(rng.integers(0, _n_scalars(protocol, b))))
            slot[int(rng.integers(1, 32))] ^= 1 << int(rng.integers(0, 8))
    # malformed: an off-curve round point on the batch's LAST instance (the one a short grid would drop), a coordinate = p just behind
    # the first block, a scalar = n at a random place
    rounds = case["rounds"]
    free = [i for i in (int(v) for v in rng.integers(1, n - 2, 8)) if i not in tampered and i != 65]
    malformed = [n - 1, 65, free[0]]
    _round_point(protocol, b, n - 1, int(rng.integers(0, rounds)))[63] ^= 1
    _round_point(protocol, b, 65, int(rng.integers(0, rounds)))[0:32] = np.frombuffer(FIELD_P.to_bytes(32, "big"), np.uint8)
    _scalar_slot(protocol, b, free[0], int(rng.integers(0, _n_scalars(protocol, b))))[:] = np.frombuffer(O.N.to_bytes(32, "big"), np.uint8)
    bad = sorted(set(tampered) | set(malformed))
    acc, flag = np.ones(n, np.uint8), np.zeros(n, bool)
    for i, rc in zip(bad, _oracle_map(lambda i: _oracle_rc(protocol, b, i), bad)):
        acc[i], flag[i] = (1 if rc == 1 else 0), rc < 0
    b.update(expect_acc=acc, expect_flag=flag, bad=bad, tampered=tampered, malformed=malformed)
    return b
