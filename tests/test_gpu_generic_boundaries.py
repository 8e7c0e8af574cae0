"""Every size threshold of the generic verifiers' launch choices (bp_pp_amd/csrc/plan_core.h: plan_generic -- table parts, round group,
final-scalars group, wavefront sums, and the reciprocal verifier's one-lane sums / phase-1 group / beside, the circuit verifier's
per_point) at T - 1, T, T + 1 instances on the GPU, against the oracle on ALL n instances (tests/generic_batches.py), with the form the
call took ("last_generic_form" of bppp_ctx_get_option) asserted against a table written by hand from that function's comments
(tests/generic_forms.py, which lists the thresholds): an off-by-one in a threshold, a grid that drops the ragged last block or the last
lane group, or a form that is never entered fails here.
The twin of tests/test_gpu_plan_boundaries.py (the u64 verifier); tests/test_generic_batches.py checks the batches themselves on the CPU,
tests/test_generic_plan.py the pure function against the same table.
WNLA (16 + 32 generators) has 4 rounds, the circuit `mixed_k2` 2 (so its lg is clipped to 1), the reciprocal (32, 16) shape 5."""
import numpy as np
import pytest

import generic_batches as GB
from generic_forms import L1, L8, N_FORMS, RECIP_ONLY, THRESHOLDS, W, expected_form

pytestmark = pytest.mark.gpu

HOST_SIZES = [(1, 1), (4, 1), (8, 1)]       # the host-buffer entry points: S + 1, 4 S + 1, 8 S + 1
TIMED_SIZES = [(64, 1), (4, 0)]


CASES = [(p, T, d) for p in GB.PROTOCOLS for T in THRESHOLDS + ([RECIP_ONLY] if p == "recip" else []) for d in (-1, 0, 1)]

_seen = {}          # (protocol, T, d) -> the form the device-resident call took


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
