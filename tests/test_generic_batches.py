"""CPU tier: the batches tests/test_gpu_generic_boundaries.py hands to the generic verifiers (tests/generic_batches.py) are what they
claim to be -- every pool entry accepted by the oracle, the corrupted set a mix of flagged and plainly rejected instances with accepted
neighbours, and the whole thing a function of (protocol, n) alone."""
import numpy as np
import pytest

import generic_batches as GB

N = 1025


@pytest.fixture(scope="module")
def batches(oracle_c):
    return {p: GB.build(p, N) for p in GB.PROTOCOLS}


@pytest.mark.parametrize("protocol", GB.PROTOCOLS)
def test_the_oracle_accepts_every_pool_entry(oracle_c, protocol):
    case = GB.pool(protocol)
    assert GB.pool_verdicts(protocol, case) == [1] * GB.POOL
    rows = case["proof_x"] if protocol == "wnla" else case["proofs"]
    assert len({r.tobytes() for r in rows}) == GB.POOL          # 257 DISTINCT instances
    assert case["rounds"] == {"wnla": 4, "circuit": 2, "recip": 5}[protocol]


@pytest.mark.parametrize("protocol", GB.PROTOCOLS)
def test_the_corrupted_set_is_flagged_rejected_and_surrounded_by_accepted_instances(batches, protocol):
    b = batches[protocol]
    acc, flag, bad = b["expect_acc"], b["expect_flag"], b["bad"]
    assert acc.shape == (N,) and flag.shape == (N,)
    clean = np.ones(N, bool)
    clean[bad] = False
    assert acc[clean].all() and not flag[clean].any()
    assert not acc[flag].any()                                   # a flagged instance is never accepted
    assert int(flag.sum()) >= 3 and flag[N - 1] and all(flag[i] for i in b["malformed"])
    assert int(((acc == 0) & ~flag).sum()) >= 20
    assert not acc[bad].any()                                    # every corruption is one the oracle notices
    for i in (0, 63, 64, N - 2, N - 1) + tuple(GB.last_wavefront_first(N, g) for g in GB.GROUP_SIZES):
        assert acc[i] == 0, i
    assert any(acc[i] == 0 and acc[i - 1] == 1 and acc[i + 1] == 1 for i in range(1, N - 1))


@pytest.mark.parametrize("protocol", GB.PROTOCOLS)
def test_the_builder_is_deterministic_in_protocol_and_size(batches, protocol):
    a, b = batches[protocol], GB.build(protocol, N)
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert (v == b[k]).all(), k
    assert a["bad"] == b["bad"]
    other = GB.build(protocol, N + 1)
    assert other["bad"] != a["bad"]                              # seeded by n as well
    assert [GB.build(p, N)["bad"] for p in GB.PROTOCOLS].count(a["bad"]) == 1      # ... and by the protocol
