"""The mixed-value-count wire expansion on the CPU: wire_mixed_expand_lane (bp_pp_amd/csrc/wire_mixed_core.h), the lane function of
k_wire_expand_mixed, compiled with g++ (tests/emul/wire_mixed_emul.cpp) and run over every lane of the wire batch
(tests/agg_mixed_wire_cases.py), against the Python expansion of the same bytes; and the conditions of that batch itself, on the oracle
alone.  The emulation works through buffers that end at an inaccessible page: a read or write behind a buffer ends the process."""
import numpy as np
import pytest

import agg_mixed_cases as M
import agg_mixed_wire_cases as MW
from emul.build_wire_mixed import load

# the small context shapes of M.CONTEXTS: chunk edges at 5 / 6 / 7 points, lane-group runs, np = nd + 1
SHAPES = [(3, 4, 4), (7, 3, 4), (6, 2, 3)]
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def emul():
    return load("host")


def run(emul, case_max, ks, C33, Q33, descending):
    """The lane function over every lane, into slots pre-filled with the sentinel -> (C64 [n, k_max, 64], Q64 [n, proof_bytes(k_max)])"""
    n, k_max = len(ks), case_max["k"]
    C64 = np.full((n, k_max, 64), SENTINEL, np.uint8)
    Q64 = np.full((n, case_max["proof_bytes"]), SENTINEL, np.uint8)
    c33, q33, kk = np.ascontiguousarray(C33).reshape(-1), np.ascontiguousarray(Q33).reshape(-1), np.ascontiguousarray(ks, np.uint8)
    rc = emul.emul_wire_expand_mixed(c33.ctypes.data, c33.size, q33.ctypes.data, q33.size, C64.ctypes.data, Q64.ctypes.data, kk.ctypes.data, n,
                                     k_max, case_max["rounds"], MW.n_scalars(case_max), int(descending))
    assert rc == 0
    return C64, Q64


def assert_expansion(case_max, ks, C64, Q64, wantC, wantQ, tag):
    """The used bytes of every slot are the expected expansion's; every other byte still holds the sentinel."""
    mC, mQ = MW.used_masks(case_max, ks)
    for got, want, mask, name in ((C64, wantC, mC, "commitments"), (Q64, wantQ, mQ, "proofs")):
        rows = np.flatnonzero(((got != want) & mask).reshape(len(ks), -1).any(axis=1))
        assert rows.size == 0, (tag, name, "used bytes differ at rows", rows[:8].tolist())
        assert (got[~mask] == SENTINEL).all(), (tag, name, "a byte no instance uses was written")


@pytest.mark.parametrize("shape", list(M.CONTEXTS))
def test_the_oracle_alone_settles_the_wire_batch(shape):
    """All but eight rows expand to the golden row's used bytes and keep its verdict; the eight are the six undecodable rows and the
    two wrong_k rows (wire_batch asserts it), and the oracle rejects each of them."""
    case_max, ks, C33, Q33, C64, Q64, exp_acc, exp_flag, notes, asked = MW.wire_batch(shape)
    assert Q33.shape[1] == MW.sec1_bytes(case_max, shape[0]) and C33.shape == (M.ROWS, shape[0], 33)
    assert len(asked) == MW.ASKED <= 8 and not exp_acc[list(asked)].any()
    what = dict(notes)
    ff = [r for r, name in notes if name == "unused_ff"][0]
    k = int(ks[ff])
    assert (C33[ff, k:] == 0xFF).all() and (Q33[ff, MW.sec1_bytes(case_max, k):] == 0xFF).all()
    assert all(exp_acc[r] == 1 for r in range(M.ROWS) if what.get(r, "clean") in ("clean", "unused_ff", "unused_other"))
    golden = M.batch(shape)
    keep = np.setdiff1d(np.arange(M.ROWS), asked)
    assert (exp_acc[keep] == golden[4][keep]).all() and (exp_flag[keep] == golden[5][keep]).all()


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_lane_of_the_wire_batch(emul, shape, descending):
    case_max, ks, C33, Q33, wantC, wantQ = MW.wire_batch(shape)[:6]
    n = M.ROWS
    lanes = emul.emul_wire_mixed_lanes(n, shape[0], case_max["rounds"], MW.n_scalars(case_max))
    assert lanes == n * (shape[0] + MW.n_points(case_max, shape[0]) + 8 * MW.n_scalars(case_max))
    C64, Q64 = run(emul, case_max, ks, C33, Q33, descending)
    assert_expansion(case_max, ks, C64, Q64, wantC, wantQ, (shape, descending))


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_counts_outside_the_range_expand_as_one_value_inside_their_slot(emul, shape, descending):
    """ks[i] = 0, k_max + 1 and 255 at clean and corrupted rows and at the last row, whose 33-byte slots are cut to what a one-value
    instance uses and end at the guard page."""
    case_max, bad, flatC, flatQ, wantC, wantQ, rows = MW.bad_count_batch(shape)
    assert flatC.size < M.ROWS * shape[0] * 33 and flatQ.size < M.ROWS * MW.sec1_bytes(case_max, shape[0])
    assert (MW.used_k(bad, shape[0])[rows] == 1).all()
    C64, Q64 = run(emul, case_max, bad, flatC, flatQ, descending)
    assert_expansion(case_max, bad, C64, Q64, wantC, wantQ, (shape, descending, "bad counts"))
    one = MW.n_points(case_max, 1)
    for r in rows:                                  # a one-value instance: l | n right behind 4 + 2 rounds + 1 points
        assert (Q64[r, 64 * one + 32 * MW.n_scalars(case_max):] == SENTINEL).all() and (C64[r, 1:] == SENTINEL).all()
