"""GPU tier of the reduction-fused Jacobian formulas (csrc/point.h: ptj_dbl with fe_mul_add_sqr, six reductions instead of seven).
Every shared-doubling sum of the u64 verifier goes through them, so the bar is the verifier's own: accept bits, status words and the
trace of challenges and hashed commitments equal the oracle's, byte for byte.  192 proofs are three wavefronts of the one-lane kernels;
a call of 2 proofs takes the small-call path, and with BPPP_NO_SPLIT the lane-group kernels, which share the same formulas."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("these tests need a GPU (they are selected with -m gpu only on the GPU box)")
    return torch


@pytest.fixture(scope="module")
def batch(oracle_c):
    """192 proofs, one in 8 corrupted, with the oracle's verdicts and traces (computed once, read-only)."""
    import workload
    gens, V, P, _ = workload.make_batch(192, first=123000)
    P, expect = workload.corrupt(P, V, every=8)
    V.setflags(write=False)
    P.setflags(write=False)
    oacc, ost = oracle_c.u64_verify_batch(gens, workload.LABEL, V, P, nthreads=min(16, os.cpu_count() or 1))
    assert (oacc == expect).all() and not ost.any() and int((expect == 0).sum()) == 24
    sample = sorted(set(range(0, 192, 8)) | set(range(1, 192, 13)) | {7, 63, 64, 65, 127, 128, 191})   # every corrupted proof + neighbours of the wave edges
    traces = {k: oracle_c.u64_verify(gens, workload.LABEL, bytes(V[k]), bytes(P[k]), trace=True) for k in sample}
    return gens, V, P, expect, traces


def _make_proto(gens, switch=None):
    import workload
    from bp_pp_amd import U64RangeProofProtocol
    g, gv, hv = workload.split_generators(gens)
    if switch:
        os.environ[switch] = "1"
    try:
        return U64RangeProofProtocol(g, gv, hv, device=0, fb_window_bits=8)
    finally:
        if switch:
            os.environ.pop(switch, None)


def _device_verify(torch, proto, label, V, P):
    n = V.shape[0]
    dV = torch.from_numpy(np.ascontiguousarray(V).copy()).cuda()
    dP = torch.from_numpy(np.ascontiguousarray(P).copy()).cuda()
    dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dS = torch.zeros(n, dtype=torch.int32, device="cuda")
    dT = torch.zeros((n, 704), dtype=torch.uint8, device="cuda")
    dR = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    proto.verify_batch_device(label, n, dV.data_ptr(), dP.data_ptr(), dA.data_ptr(), dS.data_ptr(), dT.data_ptr(), dR.data_ptr())
    torch.cuda.synchronize()
    return dA.cpu().numpy(), dS.cpu().numpy(), dT.cpu().numpy(), int(dR.item())


@pytest.mark.parametrize("switch", [None, "BPPP_NO_SPLIT", "BPPP_NO_LANE_GROUPS"])
def test_192_proofs_bit_exact_vs_oracle(torch_mod, batch, switch):
    import workload
    gens, V, P, expect, traces = batch
    proto = _make_proto(gens, switch)
    try:
        acc, st, tr, rej = _device_verify(torch_mod, proto, workload.LABEL, V, P)
    finally:
        proto.close()
    assert (acc == expect).all() and not st.any() and rej == 24
    for k, (rc, otr) in traces.items():
        assert rc == int(expect[k]) and bytes(tr[k]) == otr, k


@pytest.mark.parametrize("switch", [None, "BPPP_NO_SPLIT"])
def test_two_proofs_bit_exact_vs_oracle(torch_mod, batch, switch):
    """One honest and one corrupted proof in a call of two (proofs 7 and 8 of the batch)."""
    import workload
    gens, V, P, expect, traces = batch
    assert expect[7] == 1 and expect[8] == 0
    proto = _make_proto(gens, switch)
    try:
        acc, st, tr, rej = _device_verify(torch_mod, proto, workload.LABEL, V[7:9], P[7:9])
    finally:
        proto.close()
    assert acc.tolist() == [1, 0] and not st.any() and rej == 1
    assert bytes(tr[0]) == traces[7][1] and bytes(tr[1]) == traces[8][1]
