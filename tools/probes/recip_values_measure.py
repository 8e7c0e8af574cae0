"""What the reciprocal prover from integers costs next to the path it replaces: (32, 16) -- 128-bit values as 32 hex digits -- at 2^14
instances, three ways in ONE process on one GPU:

  1. witness on the host: numpy builds the digits and multiplicities, then commit_value_batch (bppp_msm_batch) and prove_batch
     (bppp_reciprocal_prove_batch) from host buffers -- the only path before the prove_values calls existed;
  2. prove_values_batch (bppp_reciprocal_prove_values_batch) from host buffers;
  3. prove_values_batch_seeded_device (everything resident, the draws made on the device), ended by a stream synchronise.

The three are checked against each other first (same commitments; 1 and 2 the same proofs; every proof of 3 accepted), each is warmed
up, then `--passes` alternating passes of `--steps` calls each are timed with the host clock around calls that end in a stream
synchronise; per path the median pass and the spread (max - min) / median of its passes are reported.  One more pass of path 2 with
per-kernel HIP events on gives the witness and commitment kernels' share of the launch chain.

    python tools/probes/recip_values_measure.py out.json [--n 16384] [--steps 3] [--passes 5] [--fb-window-bits 16]
    BPPP_LIB=/path/to/earlier/libbppp_hip.so python tools/probes/recip_values_measure.py out_before.json --baseline-only

--baseline-only times path 1 alone: for a build of the library from before the prove_values calls existed (given through BPPP_LIB), the
baseline the other two are compared with.

Writes one JSON document to the path given; docs/design/07-prover-and-recip256.md has the section its numbers belong in."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]

import numpy as np
import torch

from bp_pp_amd import derive_generators
from bp_pp_amd.wnla import ReciprocalRangeProofProtocol

SEED = bytes(range(32))
LABEL = b"reciprocal values probe"


def host_witness(x: np.ndarray, nd: int):
    """digits [n, nd, 32] and multiplicities [n, 16, 32] of the hex digits of x [n, 32] (big-endian), vectorised."""
    n = x.shape[0]
    nib = np.empty((n, 64), np.uint8)                 # least significant first
    rev = x[:, ::-1]
    nib[:, 0::2], nib[:, 1::2] = rev & 15, rev >> 4
    assert not nib[:, nd:].any(), "a value has more than dim_nd hex digits"
    digits = np.zeros((n, nd, 32), np.uint8)
    digits[:, :, 31] = nib[:, :nd]
    m = np.zeros((n, 16, 32), np.uint8)
    m[:, :, 31] = (nib[:, :nd, None] == np.arange(16, dtype=np.uint8)[None, None, :]).sum(axis=1)
    return digits, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--n", type=int, default=1 << 14)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--fb-window-bits", type=int, default=16)
    ap.add_argument("--baseline-only", action="store_true")
    args = ap.parse_args()
    if torch.cuda.device_count() == 0:
        sys.exit("needs a GPU: nothing here is measured without one")
    nd, npp, n = 32, 16, args.n
    NG, NH = 32, 64
    raw = derive_generators(b"bppp-probe-recip-values", 1 + NG + NH)
    pts = [raw[64 * i:64 * i + 64] for i in range(1 + NG + NH)]
    proto = ReciprocalRangeProofProtocol(nd, npp, pts[0], pts[1:1 + nd], pts[1 + NG:1 + NG + nd + 10], pts[1 + nd:1 + NG],
                                         pts[1 + NG + nd + 10:], device=0, fb_window_bits=args.fb_window_bits)
    rng = np.random.default_rng(20261)
    x = np.zeros((n, 32), np.uint8)
    x[:, 16:] = rng.integers(0, 256, (n, 16), dtype=np.uint8)        # 128-bit values
    s = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    s[:, 0] &= 0x7F                                                  # canonical
    rnd = rng.integers(0, 256, (n, 20 + 2 * nd, 32), dtype=np.uint8)
    rnd[:, :, 0] &= 0x7F
    dX, dS = torch.from_numpy(x).cuda(), torch.from_numpy(s).cuda()
    shape = proto._proof_shape()
    dP = torch.zeros((n, proto.proof_bytes()), dtype=torch.uint8, device="cuda")
    dC = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    dSt = torch.zeros(n, dtype=torch.int32, device="cuda")

    def path1():
        digits, m = host_witness(x, nd)
        com, cst = proto.commit_value_batch(x, s)
        proofs, st, _ = proto.prove_batch(LABEL, com, x, s, digits, m, rnd)
        return proofs, com, st

    def path2():
        proofs, com, st, _ = proto.prove_values_batch(LABEL, x, s, rnd)
        return proofs, com, st

    def path3():
        proto.prove_values_batch_seeded_device(LABEL, n, dX.data_ptr(), dS.data_ptr(), SEED, 0, dP.data_ptr(), dC.data_ptr(), dSt.data_ptr())
        proto.synchronize()

    # the three agree (this is also the warm-up of every path)
    p1, c1, st1 = path1()
    assert not st1.any()
    paths = {"host_witness_commit_prove": path1}
    if not args.baseline_only:
        p2, c2, st2 = path2()
        path3()
        assert not st2.any() and not dSt.cpu().numpy().any()
        assert (p1 == p2).all() and (c1 == c2).all() and (dC.cpu().numpy() == c1).all()
        paths.update({"prove_values_batch": path2, "prove_values_batch_seeded_device": path3})
    acc, vst = proto.verify_batch(LABEL, c1, p1 if args.baseline_only else dP.cpu().numpy(), *shape)
    assert acc.all() and not vst.any()
    for f in paths.values():
        f()
    times = {k: [] for k in paths}
    for _ in range(args.passes):
        for k, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / args.steps * 1e3)
    res = {"shape": [nd, npp], "n": n, "steps": args.steps, "passes": args.passes, "fb_window_bits": proto.get_option("fb_window_bits"),
           "ms_per_call": {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / statistics.median(v),
                               "passes": v} for k, v in times.items()}}
    host_only = []
    for _ in range(args.passes):
        t0 = time.perf_counter()
        host_witness(x, nd)
        host_only.append((time.perf_counter() - t0) * 1e3)
    res["host_witness_ms"] = statistics.median(host_only)
    if not args.baseline_only:
        proto.enable_timing(True)
        proto.timings(reset=True)
        for _ in range(args.steps):
            path2()
        kt = proto.timings(reset=True)
        proto.enable_timing(False)
        ms = {k: v["total_ms"] / args.steps for k, v in kt.items() if v["launches"]}
        chain = sum(ms.values())
        res["kernels_ms_per_call"] = ms
        res["witness_share_of_chain"] = ms.get("k_rprove_witness", 0.0) / chain if chain else None
        res["witness_and_commit_share_of_chain"] = (ms.get("k_rprove_witness", 0.0) + ms.get("k_rprove_commit", 0.0)) / chain if chain else None
    proto.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "ms_per_call"} | {"median_ms": {k: v["median"] for k, v in res["ms_per_call"].items()},
                                                                           "spread": {k: v["spread"] for k, v in res["ms_per_call"].items()}}))


if __name__ == "__main__":
    main()
