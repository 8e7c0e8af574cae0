"""The product's own k_wire_expand_mixed on the device, on results: bp_pp_amd/csrc/k_wire_mixed.hip included as it is in a test-only
library with a C runner over device pointers (tests/emul/wire_mixed_device.hip, built by tests/emul/build_wire_mixed.py), run over the
wire batch (tests/agg_mixed_wire_cases.py) at the four context shapes of agg_mixed_cases.CONTEXTS.  The assertions are those of the
CPU emulation (tests/test_agg_mixed_wire_emul.py): the used bytes of every slot are the Python expansion, every other byte of the
pre-filled 64-byte slots still holds 0xA5, and counts outside [1, k_max] expand as one-value instances."""
import numpy as np
import pytest

import agg_mixed_cases as M
import agg_mixed_wire_cases as MW
from test_agg_mixed_wire_emul import SENTINEL, assert_expansion

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runner():
    import torch
    if torch.cuda.device_count() == 0:
        pytest.fail("needs a GPU")
    from emul.build_wire_mixed import load
    return load("gfx950")


def run(runner, case_max, ks, C33, Q33):
    import torch
    n, k_max = len(ks), case_max["k"]
    up = lambda a: torch.from_numpy(np.array(a, np.uint8, copy=True).reshape(-1)).cuda()
    dC33, dQ33, dK = up(C33), up(Q33), up(ks)
    dC64 = torch.full((n * k_max * 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    dQ64 = torch.full((n * case_max["proof_bytes"],), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = runner.wire_mixed_run_device(dC33.data_ptr(), dQ33.data_ptr(), dC64.data_ptr(), dQ64.data_ptr(), dK.data_ptr(), n, k_max,
                                      case_max["rounds"], MW.n_scalars(case_max))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dC64.cpu().numpy().reshape(n, k_max, 64), dQ64.cpu().numpy().reshape(n, -1)


@pytest.mark.parametrize("shape", list(M.CONTEXTS))
def test_the_wire_batch_expands_to_the_python_expansion(runner, shape):
    case_max, ks, C33, Q33, wantC, wantQ = MW.wire_batch(shape)[:6]
    C64, Q64 = run(runner, case_max, ks, C33, Q33)
    assert_expansion(case_max, ks, C64, Q64, wantC, wantQ, shape)


@pytest.mark.parametrize("shape", list(M.CONTEXTS))
def test_counts_outside_the_range_expand_as_one_value_inside_their_slot(runner, shape):
    """The 33-byte buffers are cut to what the last row uses as a one-value instance: the kernel is given no byte more."""
    case_max, bad, flatC, flatQ, wantC, wantQ, rows = MW.bad_count_batch(shape)
    C64, Q64 = run(runner, case_max, bad, flatC, flatQ)
    assert_expansion(case_max, bad, C64, Q64, wantC, wantQ, (shape, "bad counts"))
    assert (C64[rows, 1:] == SENTINEL).all()
