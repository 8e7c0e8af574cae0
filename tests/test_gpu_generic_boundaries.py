"""Every size threshold of the generic verifiers' launch choices (bp_pp_amd/csrc/bppp_generic.hip: wnla_table_parts, wnla_round_group,
wnla_final_scalars_group_lg, generic_fb_wide, and the reciprocal verifier's fb_one_lane / phase-1 group / beside, the circuit verifier's
per_point) at T - 1, T, T + 1 instances on the GPU, against the oracle on ALL n instances (tests/generic_batches.py), with the form the
call took ("last_generic_form" of bppp_ctx_get_option) asserted against a table written by hand from those predicates' comments: an
off-by-one in a threshold, a grid that drops the ragged last block or the last lane group, or a form that is never entered fails here.
The twin of tests/test_gpu_plan_boundaries.py (the u64 verifier); tests/test_generic_batches.py checks the batches themselves on the CPU.

Sizes are in units of S = "n_simds" (1,024 on an MI355X), blocks = ceil(n / 64):
    tables in 4 | 2 | 1 parts, rounds on 16 | 8 lanes                 n <= S | n <= 4 S
    rounds on 4 | 2 | 1 lanes (one set of tables)                     4 blocks <= S | 2 blocks <= S         = n <= 16 S | 32 S
    final scalars on 8 | 4 | 2 | 1 lanes (lg 3 | 2 | 1 | 0)           blocks << (lg + 1) <= 4 S             = n <= 32 S | 64 S | 128 S,
                                                                      and lg <= rounds - 1
    fixed-base sums on a wavefront | 8 lanes per instance             n <= 8 S
    reciprocal: fixed-base sums on one lane                           n >= 128 S
    reciprocal: phase 1 on 8 | 4 | 2 | 1 lanes                        2 G blocks <= S                       = n <= 8 S | 16 S | 32 S
    reciprocal: tables and C0's sum beside phase 1                    2 blocks <= S (timing off)            = n <= 32 S
    circuit: C0's variable-base sum on a lane per point (L = 8)       L blocks <= 2 S                       = n <= 16 S
WNLA (16 + 32 generators) has 4 rounds, the circuit `mixed_k2` 2 (so its lg is clipped to 1), the reciprocal (32, 16) shape 5."""
import numpy as np
import pytest

import generic_batches as GB

pytestmark = pytest.mark.gpu

THRESHOLDS = [1, 4, 8, 16, 32, 64]          # x S
RECIP_ONLY = 128                            # x S: the one-lane fixed-base sums
HOST_SIZES = [(1, 1), (4, 1), (8, 1)]       # the host-buffer entry points: S + 1, 4 S + 1, 8 S + 1
TIMED_SIZES = [(64, 1), (4, 0)]


def F(tab_parts, round_group, lg, fixed_base, phase1_group=0, beside=0, per_point=0):
    return dict(tab_parts=tab_parts, round_group=round_group, final_scalars_lg=lg, fixed_base=fixed_base, phase1_group=phase1_group,
                beside=beside, parts=1, per_point=per_point)


W, L8, L1 = "wavefront", "lanes8", "one_lane"
# (protocol, T in S) -> the form at T - 1, T, T + 1 instances.  Written by hand from the list above; NOT computed from n.
FORMS = {
    ("wnla", 1): (F(4, 16, 3, W), F(4, 16, 3, W), F(2, 8, 3, W)),
    ("wnla", 4): (F(2, 8, 3, W), F(2, 8, 3, W), F(1, 4, 3, W)),
    ("wnla", 8): (F(1, 4, 3, W), F(1, 4, 3, W), F(1, 4, 3, L8)),
    ("wnla", 16): (F(1, 4, 3, L8), F(1, 4, 3, L8), F(1, 2, 3, L8)),
    ("wnla", 32): (F(1, 2, 3, L8), F(1, 2, 3, L8), F(1, 1, 2, L8)),
    ("wnla", 64): (F(1, 1, 2, L8), F(1, 1, 2, L8), F(1, 1, 1, L8)),
    # two rounds: the final scalars split in two at most (lg 1) at every size of the sweep
    ("circuit", 1): (F(4, 16, 1, W, per_point=1), F(4, 16, 1, W, per_point=1), F(2, 8, 1, W, per_point=1)),
    ("circuit", 4): (F(2, 8, 1, W, per_point=1), F(2, 8, 1, W, per_point=1), F(1, 4, 1, W, per_point=1)),
    ("circuit", 8): (F(1, 4, 1, W, per_point=1), F(1, 4, 1, W, per_point=1), F(1, 4, 1, L8, per_point=1)),
    ("circuit", 16): (F(1, 4, 1, L8, per_point=1), F(1, 4, 1, L8, per_point=1), F(1, 2, 1, L8)),
    ("circuit", 32): (F(1, 2, 1, L8), F(1, 2, 1, L8), F(1, 1, 1, L8)),
    ("circuit", 64): (F(1, 1, 1, L8), F(1, 1, 1, L8), F(1, 1, 1, L8)),
    ("recip", 1): (F(4, 16, 3, W, 8, 1), F(4, 16, 3, W, 8, 1), F(2, 8, 3, W, 8, 1)),
    ("recip", 4): (F(2, 8, 3, W, 8, 1), F(2, 8, 3, W, 8, 1), F(1, 4, 3, W, 8, 1)),
    ("recip", 8): (F(1, 4, 3, W, 8, 1), F(1, 4, 3, W, 8, 1), F(1, 4, 3, L8, 4, 1)),
    ("recip", 16): (F(1, 4, 3, L8, 4, 1), F(1, 4, 3, L8, 4, 1), F(1, 2, 3, L8, 2, 1)),
    ("recip", 32): (F(1, 2, 3, L8, 2, 1), F(1, 2, 3, L8, 2, 1), F(1, 1, 2, L8, 1, 0)),
    ("recip", 64): (F(1, 1, 2, L8, 1, 0), F(1, 1, 2, L8, 1, 0), F(1, 1, 1, L8, 1, 0)),
    ("recip", 128): (F(1, 1, 1, L8, 1, 0), F(1, 1, 1, L1, 1, 0), F(1, 1, 0, L1, 1, 0)),
}
# distinct forms per sweep.  WNLA: {4 parts; 2 parts; group 4 + wavefront sum; group 4 + 8-lane sum; group 2; group 1 with the final
# scalars on 4 lanes; the same on 2 lanes} (final scalars on ONE lane start beyond 128 S: only the reciprocal sweep goes there).
# Circuit: the round count clips lg to 1, so the last two of those are one form, and both per_point values are among the six.
# Reciprocal: those seven, 128 S on the one-lane fixed-base sums, 128 S + 1 with one-lane final scalars as well; G = 8, 4, 2, 1 and
# both `beside` values among them.
N_FORMS = {"wnla": 7, "circuit": 6, "recip": 9}
PROTOCOL_NAME = {"wnla": "wnla", "circuit": "circuit", "recip": "reciprocal"}
CASES = [(p, T, d) for p in GB.PROTOCOLS for T in THRESHOLDS + ([RECIP_ONLY] if p == "recip" else []) for d in (-1, 0, 1)]

_seen = {}          # (protocol, T, d) -> the form the device-resident call took


def expected_form(protocol, T, d):
    return dict(FORMS[(protocol, T)][d + 1], protocol=PROTOCOL_NAME[protocol])


@pytest.fixture(scope="module")
def verifiers():
    """One context per protocol over the pools' generators (the reciprocal one as tests/test_gpu_recip.py makes its generic contexts)."""
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    from bp_pp_amd.wnla import ArithmeticCircuit, ReciprocalRangeProofProtocol, WeightNormLinearArgument
    made = {}
    try:
        cw = GB.pool("wnla")
        made["wnla"] = WeightNormLinearArgument(cw["g"], cw["gv"], cw["hv"], device=0, fb_window_bits=16)
        cc = GB.pool("circuit")
        part = lambda typ, j: (None if cc["part"][typ][j] < 0 else int(cc["part"][typ][j]))
        arr = lambda b: np.frombuffer(b, np.uint8).reshape(-1, 32)
        made["circuit"] = ArithmeticCircuit(cc["nm"], cc["no"], cc["k"], cc["nv"], cc["g"], cc["gv"], cc["hv"], arr(cc["Wm_bytes"]),
                                            arr(cc["Wl_bytes"]), arr(cc["am_bytes"]), arr(cc["al_bytes"]), cc["f_l"], cc["f_m"], cc["gv_"],
                                            cc["hv_"], part, device=0, fb_window_bits=16)
        cr = GB.pool("recip")
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("BPPP_GENERIC_U64_SHAPE", "1")
            made["recip"] = ReciprocalRangeProofProtocol(cr["nd"], cr["np"], cr["g"], cr["gv"], cr["hv"], cr["gv_"], cr["hv_"], device=0,
                                                         fb_window_bits=16)
        for v in made.values():
            assert _w(v).generic_form() == {} and _w(v).get_option("last_generic_form") == 0
        S = made["wnla"].get_option("n_simds")
        assert S >= 64 and S % 64 == 0 and all(_w(v).get_option("n_simds") == S for v in made.values())
        made["S"] = S
        yield made
    finally:
        for k, v in made.items():
            if k != "S":
                v.close()


def _w(verifier):
    return getattr(verifier, "_w", verifier)


def _shape(protocol, case):
    return (case["rounds"], case["pl"], case["pn"]) if protocol == "circuit" else (case["rounds"], case["nl"], case["nn"])


def _device_verify(verifier, b):
    """The device-resident entry point (what bench.py times): inputs uploaded first, accept / status read back after the call."""
    import torch
    protocol, n, case = b["protocol"], b["n"], b["case"]
    keys = ("commitments", "c", "rho", "mu", "proof_r", "proof_x", "proof_l", "proof_n") if protocol == "wnla" else ("commitments", "proofs")
    d = {k: torch.from_numpy(b[k]).cuda() for k in keys}
    dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dS = torch.full((n,), 7, dtype=torch.int32, device="cuda")          # (an instance no kernel reached keeps the 7)
    torch.cuda.synchronize()
    rounds, nl, nn = _shape(protocol, case)
    if protocol == "wnla":
        verifier.verify_batch_device(case["label"], n, d["commitments"].data_ptr(), d["c"].data_ptr(), d["rho"].data_ptr(), d["mu"].data_ptr(),
                                     rounds, d["proof_r"].data_ptr(), d["proof_x"].data_ptr(), d["proof_l"].data_ptr(), nl,
                                     d["proof_n"].data_ptr(), nn, dA.data_ptr(), dS.data_ptr())
    else:
        verifier.verify_batch_device(case["label"], n, d["commitments"].data_ptr(), d["proofs"].data_ptr(), rounds, nl, nn, dA.data_ptr(),
                                     dS.data_ptr())
    verifier.synchronize()
    torch.cuda.synchronize()
    return dA.cpu().numpy(), dS.cpu().numpy()


def _host_verify(verifier, b):
    protocol, case = b["protocol"], b["case"]
    if protocol == "wnla":
        return verifier.verify_batch(case["label"], **{k: b[k] for k in ("commitments", "c", "rho", "mu", "proof_r", "proof_x", "proof_l", "proof_n")})
    return verifier.verify_batch(case["label"], b["commitments"], b["proofs"], *_shape(protocol, case))


def _assert_verdicts(b, acc, st, what):
    """All n accept bits equal the oracle's; the statuses are zero exactly where the oracle raised no encoding error; the last
    instance -- the one a short grid drops -- is flagged."""
    n, tag = b["n"], (b["protocol"], b["n"], what)
    assert acc.shape == (n,) and st.shape == (n,)
    wrong = np.flatnonzero(acc != b["expect_acc"])
    assert wrong.size == 0, (tag, "accept bits differ at", wrong[:16].tolist(), "of", int(wrong.size), "corrupted:", b["bad"])
    wrong = np.flatnonzero((st != 0) != b["expect_flag"])
    assert wrong.size == 0, (tag, "statuses differ at", wrong[:16].tolist(), st[wrong[:16]].tolist(), "malformed:", b["malformed"])
    assert st[n - 1] != 0 and acc[n - 1] == 0, tag
    assert int((st != 0).sum()) >= 3 and int(((acc == 0) & (st == 0)).sum()) >= 20, tag


def _run_case(verifiers, protocol, T, d):
    n = T * verifiers["S"] + d
    b = GB.build(protocol, n)
    v = verifiers[protocol]
    acc, st = _device_verify(v, b)
    form = _w(v).generic_form()
    _assert_verdicts(b, acc, st, "device")
    assert form == expected_form(protocol, T, d), (protocol, T, d, form)
    _seen[(protocol, T, d)] = tuple(sorted(form.items()))
    return b, acc, st


@pytest.mark.parametrize("protocol,T,d", CASES)
def test_generic_verify_at_every_threshold_vs_oracle(verifiers, protocol, T, d):
    _run_case(verifiers, protocol, T, d)


@pytest.mark.parametrize("T,d", HOST_SIZES)
@pytest.mark.parametrize("protocol", ["wnla", "circuit"])
def test_host_buffer_entry_just_past_a_threshold_vs_oracle(verifiers, protocol, T, d):
    """bppp_wnla_verify_batch / bppp_circuit_verify_batch (upload, verify, download in one call) at the first size of the 2-part,
    the 4-lane and the 8-lane-sum forms."""
    b = GB.build(protocol, T * verifiers["S"] + d)
    acc, st = _host_verify(verifiers[protocol], b)
    form = _w(verifiers[protocol]).generic_form()
    _assert_verdicts(b, acc, st, "host")
    assert form == expected_form(protocol, T, d), (protocol, T, d, form)


@pytest.mark.parametrize("T,d", TIMED_SIZES)
@pytest.mark.parametrize("protocol", GB.PROTOCOLS)
def test_kernel_timing_leaves_the_verdicts_alone(verifiers, protocol, T, d):
    """With per-kernel timing on everything runs on one stream (no `beside`, one part): the second path through the same sizes.  Accept
    bits and statuses byte-equal to the untimed call's, and k_wnla_round launched once per round."""
    b, acc, st = _run_case(verifiers, protocol, T, d)
    v = verifiers[protocol]
    v.enable_timing(True)
    try:
        v.timings()                                  # (reset)
        acc_t, st_t = _device_verify(v, b)
        kt = v.timings()
        form = _w(v).generic_form()
    finally:
        v.enable_timing(False)
    assert acc_t.tobytes() == acc.tobytes() and st_t.tobytes() == st.tobytes(), (protocol, b["n"])
    assert kt["k_wnla_round"]["launches"] == b["case"]["rounds"] and kt["k_wnla_msm"]["launches"] == 1
    assert form == dict(expected_form(protocol, T, d), beside=0), (protocol, T, d, form)


def test_every_generic_regime_was_entered(verifiers):
    """The sweep is only worth its name if its sizes span every form: the set of forms the device-resident calls took is the set the
    table holds, of the size stated above (cases the sweep above has not run in this process are run here)."""
    for protocol, T, d in CASES:
        if (protocol, T, d) not in _seen:
            _run_case(verifiers, protocol, T, d)
    for protocol in GB.PROTOCOLS:
        seen = {f for (p, _, _), f in _seen.items() if p == protocol}
        table = {tuple(sorted(expected_form(p, T, d).items())) for (p, T, d) in CASES if p == protocol}
        assert seen == table and len(seen) == N_FORMS[protocol], (protocol, len(seen), sorted(seen))
    forms = lambda p, key: {dict(f)[key] for (q, _, _), f in _seen.items() if q == p}
    assert forms("wnla", "tab_parts") == {4, 2, 1} and forms("wnla", "round_group") == {16, 8, 4, 2, 1}
    assert forms("wnla", "final_scalars_lg") == {3, 2, 1} and forms("wnla", "fixed_base") == {W, L8}
    assert forms("circuit", "per_point") == {0, 1} and forms("circuit", "final_scalars_lg") == {1}
    assert forms("recip", "phase1_group") == {8, 4, 2, 1} and forms("recip", "beside") == {0, 1}
    assert forms("recip", "fixed_base") == {W, L8, L1} and forms("recip", "final_scalars_lg") == {3, 2, 1, 0}
