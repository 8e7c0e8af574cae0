"""The WIRE batch of the mixed-value-count aggregate (bppp_reciprocal_agg_verify_batch_mixed_sec1 and its RLC forms): the batch of
tests/agg_mixed_cases.py (M.batch(shape): 71 rows, four context shapes) in 33-byte slots laid out by k_max, the expansion the device
makes of it, and the verdict expected of every row.

Packing: every row with its own value count k -- commitments wire.pack(C[row, :k], k), the proof wire.pack(Q[row, :proof_bytes(k)],
4 + 2 rounds + k, nl + nn) -- at the front of its slots.
    wrong_k_plus / wrong_k_minus  packed with the proof's TRUE k; ks[row] stays the wrong one
    unused_ff                     every byte behind its used part is 0xFF on the 33-byte side too
    unused_other                  sits in front of the packed k_max proof and commitments it sits in front of in the 64-byte batch
    R_off_curve, V_off_curve, coordinate_p (two rows each): an off-curve point has no compressed form; the row carries an undecodable
                                  encoding in the same field instead, cycling through test_gpu_generic_sec1.bad_encodings (bad tag,
                                  x = p, x = 2^256 - 1, a non-residue x)
The expected expansion is made row by row under ks[row]: wire.expand with that row's point counts, into zeroed 64-byte slots laid out
by k_max.  A row whose expansion is byte for byte the golden row's used bytes keeps the golden verdict; every other row -- they must be
exactly the six undecodable rows and the two wrong_k rows -- gets the oracle's verdict on its expansion,
A.verify(M.setup_on(case_max, ks[row]), ...)."""
import functools

import numpy as np

import agg_cases as A
import agg_mixed_cases as M
from bp_pp_amd import wire
from test_gpu_generic_sec1 import bad_encodings

OFF_CURVE_KINDS = ("R_off_curve", "V_off_curve", "coordinate_p")
UNDECODABLE = (0, 2, 3, 4)                     # bad_encodings: tag 04, x = p, x = 2^256 - 1, a non-residue x (5 is the identity)
ASKED = 8                                      # rows whose verdict is the oracle's at test time: 6 undecodable + 2 wrong_k


def n_points(case, k):
    return 4 + 2 * case["rounds"] + k


def n_scalars(case):
    return case["nl"] + case["nn"]


def sec1_bytes(case, k):
    """S(k) = bppp_reciprocal_agg_proof_sec1_bytes(k, rounds, nl, nn)"""
    return 33 * n_points(case, k) + 32 * n_scalars(case)


def shape_of(case):
    return case["rounds"], case["nl"], case["nn"]


def undecodable(valid33, i):
    return np.frombuffer(bad_encodings(bytes(valid33))[UNDECODABLE[i % len(UNDECODABLE)]][0], np.uint8)


def used_k(ks, k_max):
    """The value count an instance is read with: ks[i], or 1 where it is outside [1, k_max] (agg_mixed_k's rule)."""
    ks = np.asarray(ks).astype(np.int64)
    return np.where((ks < 1) | (ks > k_max), 1, ks)


def expand(case_max, ks, C33, Q33, fill=0):
    """The 64-byte slots the device expands a wire batch to, row by row under ks[row]; what no instance uses holds `fill`.
    -> (C64 [n, k_max, 64], Q64 [n, proof_bytes(k_max)])"""
    k_max, n = case_max["k"], len(ks)
    S = n_scalars(case_max)
    C64 = np.full((n, k_max, 64), fill, np.uint8)
    Q64 = np.full((n, case_max["proof_bytes"]), fill, np.uint8)
    for row, k in enumerate(used_k(ks, k_max).tolist()):
        P = n_points(case_max, k)
        C64[row, :k] = wire.expand(C33[row, :k].reshape(1, -1), k).reshape(k, 64)
        Q64[row, :64 * P + 32 * S] = wire.expand(Q33[row, :33 * P + 32 * S].reshape(1, -1), P, S)[0]
    return C64, Q64


def used_masks(case_max, ks):
    """Boolean masks of the bytes an instance uses of its 64-byte slots: (mC [n, k_max, 64], mQ [n, proof_bytes(k_max)])."""
    k_max, n = case_max["k"], len(ks)
    mC = np.zeros((n, k_max, 64), bool)
    mQ = np.zeros((n, case_max["proof_bytes"]), bool)
    for row, k in enumerate(used_k(ks, k_max).tolist()):
        mC[row, :k] = True
        mQ[row, :A.proof_bytes(k, *shape_of(case_max))] = True
    return mC, mQ


@functools.lru_cache(maxsize=None)
def wire_batch(shape):
    """-> (case_max, ks, C33 [ROWS, k_max, 33], Q33 [ROWS, S(k_max)], C64, Q64, expect_acc, expect_flag, notes, asked): the packed
    batch, its expected expansion (zeros behind what an instance uses), the verdicts, and the rows the oracle was asked about.  Made
    once; never written to."""
    case_max, ks, C, Q, exp_acc, exp_flag, notes = M.batch(shape)
    k_max, rounds, S = case_max["k"], case_max["rounds"], n_scalars(case_max)
    kmin, kmax = M.CONTEXTS[shape][0], M.CONTEXTS[shape][-1]
    what = dict(notes)
    true_k = ks.astype(np.int64)
    for row, name in notes:
        if name == "wrong_k_plus":
            true_k[row] = kmin
        elif name == "wrong_k_minus":
            true_k[row] = kmax
    C33 = np.zeros((M.ROWS, k_max, 33), np.uint8)
    Q33 = np.zeros((M.ROWS, sec1_bytes(case_max, k_max)), np.uint8)

    def put(row, k, c64, q64):
        P = n_points(case_max, k)
        C33[row, :k] = wire.pack(c64[:k].reshape(1, -1), k).reshape(k, 33)
        Q33[row, :33 * P + 32 * S] = wire.pack(q64[:64 * P + 32 * S].reshape(1, -1), P, S)[0]

    undecodable_rows = []
    for row in range(M.ROWS):
        name, k = what.get(row, "clean"), int(true_k[row])
        if name == "unused_ff":
            C33[row] = 0xFF
            Q33[row] = 0xFF
        elif name == "unused_other":
            put(row, kmax, *_pool_entry(shape, kmax, 0))
        put(row, k, C[row], Q[row])
        kind = name.split(",")[0]
        if kind in OFF_CURVE_KINDS:
            i = len(undecodable_rows)
            if kind == "V_off_curve":
                C33[row, k - 1] = undecodable(C33[row, k - 1], i)
            else:
                j = {"R_off_curve": 4 + 2 * rounds + k // 2, "coordinate_p": 2}[kind]
                Q33[row, 33 * j:33 * j + 33] = undecodable(Q33[row, 33 * j:33 * j + 33], i)
            undecodable_rows.append(row)
    C64, Q64 = expand(case_max, ks, C33, Q33)
    mC, mQ = used_masks(case_max, ks)
    exp_acc, exp_flag = exp_acc.copy(), exp_flag.copy()
    asked = []
    for row in range(M.ROWS):
        if (C64[row][mC[row]] == C[row][mC[row]]).all() and (Q64[row][mQ[row]] == Q[row][mQ[row]]).all():
            continue
        case, com, proof = M.row_inputs(case_max, ks, C64, Q64, row)
        rc = A.verify(case, com, proof)
        exp_acc[row], exp_flag[row] = (1 if rc == 1 else 0), rc < 0
        asked.append(row)
    wrong_k = [row for row, name in notes if name.startswith("wrong_k")]
    assert sorted(asked) == sorted(undecodable_rows + wrong_k) and len(asked) == ASKED, (shape, asked, undecodable_rows, wrong_k)
    assert all(exp_flag[r] and not exp_acc[r] for r in undecodable_rows), shape          # k256 would not have deserialised them
    for a in (C33, Q33, C64, Q64, exp_acc, exp_flag):
        a.setflags(write=False)
    return case_max, ks, C33, Q33, C64, Q64, exp_acc, exp_flag, notes, tuple(asked)


def _pool_entry(shape, k, j):
    """(commitments [k, 64], proof [proof_bytes(k)]) of the golden pool, as arrays."""
    com, proof = M.load_pool(shape)[1][k][j]
    return np.frombuffer(com, np.uint8).reshape(k, 64), np.frombuffer(proof, np.uint8)


def bad_count_batch(shape):
    """The wire batch with counts outside [1, k_max] at rows of both kinds (clean and corrupted) and at the LAST row, whose slots are
    cut to what a one-value instance uses: (case_max, ks, C33 flat bytes, Q33 flat bytes, C64, Q64 expected, rows)."""
    case_max, ks, C33, Q33 = wire_batch(shape)[:4]
    k_max = case_max["k"]
    bad = ks.copy()
    rows = [1, 6, M.CLEAN + 3, M.ROWS - 1]
    bad[1], bad[6], bad[M.CLEAN + 3], bad[M.ROWS - 1] = 0, k_max + 1, 255, k_max + 1
    C64, Q64 = expand(case_max, bad, C33, Q33, fill=0xA5)
    flatC = C33.reshape(-1)[:(M.ROWS - 1) * k_max * 33 + 33].copy()
    flatQ = Q33.reshape(-1)[:(M.ROWS - 1) * Q33.shape[1] + sec1_bytes(case_max, 1)].copy()
    return case_max, bad, flatC, flatQ, C64, Q64, rows
