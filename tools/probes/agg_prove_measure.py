"""What the aggregated reciprocal PROVER costs per VALUE next to separate u64 proofs: in ONE process on one GPU, over one pair of
contexts,

  1. 2^13 aggregated instances of (k, nd, np) = (16, 16, 16) -- 2^17 u64 values -- through
     bppp_reciprocal_agg_prove_values_batch_seeded_device;
  2. the same 2^17 values as separate proofs through bppp_u64_prove_batch_seeded_device.

Both are warmed up (every instance of both unflagged), then `--passes` alternating passes of `--steps` calls each are timed with the host
clock around calls that end in a stream synchronise; per path the median pass, (max - min) / median of its passes and VALUES per second.
One more aggregate call with per-kernel HIP events on gives the kernel table, and from it the closed-form collect's share of the chain
(k_aprove_collect: the collect run once more by itself, which the library does only while timing is on) and stage B's around it.
Nothing here sets a target: it is the record of what was measured.

    python tools/probes/agg_prove_measure.py out.json [--lg-n 13] [--steps 3] [--passes 5]

Writes one JSON document to the path given; docs/design/07-prover-and-recip256.md section 7e has its numbers."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import numpy as np
import torch

SHAPE = (16, 16, 16)
U64_LABEL = b"aggregate prove probe u64"
SEED = bytes(range(32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lg-n", type=int, default=13)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5)
    args = ap.parse_args()
    if torch.cuda.device_count() == 0:
        sys.exit("needs a GPU: nothing here is measured without one")
    import agg_golden
    import workload
    from bp_pp_amd import U64RangeProofProtocol, _build
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol
    n, k = 1 << args.lg_n, SHAPE[0]
    m = n * k
    case = agg_golden.load(SHAPE)[0]
    agg = AggregatedReciprocalRangeProofProtocol(*SHAPE, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0)
    g, gv, hv = workload.split_generators(workload.make_batch(1, first=0)[0])
    u64 = U64RangeProofProtocol(g, gv, hv, device=0)
    rng = np.random.default_rng(20263)
    vals = rng.integers(0, 1 << 63, m, dtype=np.uint64)
    x32 = np.zeros((m, 32), np.uint8)
    x32[:, 24:] = vals.astype(">u8").view(np.uint8).reshape(m, 8)            # the same values as 32-byte big-endian scalars
    s = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    s[:, 0] &= 0x7F
    dX64 = torch.from_numpy(vals.view(np.int64)).cuda()
    dX32, dSb = torch.from_numpy(x32).cuda(), torch.from_numpy(s).cuda()
    pb = agg.proof_bytes(*agg.proof_shape())
    dAP = torch.zeros((n, pb), dtype=torch.uint8, device="cuda")
    dAC = torch.zeros((n, k, 64), dtype=torch.uint8, device="cuda")
    dAS = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    dUP = torch.zeros((m, 928), dtype=torch.uint8, device="cuda")
    dUC = torch.zeros((m, 64), dtype=torch.uint8, device="cuda")
    dUS = torch.full((m,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def path_agg():
        agg.prove_values_batch_seeded_device(case["label"], n, dX32.data_ptr(), dSb.data_ptr(), SEED, 0, dAP.data_ptr(), dAC.data_ptr(),
                                             dAS.data_ptr())
        agg.synchronize()

    def path_u64():
        u64.prove_batch_seeded_device(U64_LABEL, m, dX64.data_ptr(), dSb.data_ptr(), SEED, 0, dUP.data_ptr(), dUC.data_ptr(), dUS.data_ptr())
        u64.synchronize()

    paths = {"aggregate_16x16x16": path_agg, "u64_separate": path_u64}
    for f in paths.values():                 # warm-up, and no instance of either flagged
        f()
    torch.cuda.synchronize()
    assert not dAS.cpu().numpy().any() and not dUS.cpu().numpy().any()
    # what was proved verifies (a sample: the first 256 instances), and both provers committed to the same values
    rounds, nl, nn = agg.proof_shape()
    dA = torch.zeros(256, dtype=torch.uint8, device="cuda")
    dV = torch.zeros(256, dtype=torch.int32, device="cuda")
    agg.verify_batch_device(case["label"], 256, dAC.data_ptr(), dAP.data_ptr(), rounds, nl, nn, dA.data_ptr(), dV.data_ptr())
    agg.synchronize()
    assert dA.cpu().numpy().all() and not dV.cpu().numpy().any()
    times = {name: [] for name in paths}
    for _ in range(args.passes):
        for name, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    res = {"shape": list(SHAPE), "instances": n, "values": m, "steps": args.steps, "passes": args.passes,
           "device": torch.cuda.get_device_name(0), "device_code_sha256": _build.device_code_sha256(),
           "fb_window_bits": {"aggregate": agg.get_option("fb_window_bits"), "u64": u64.get_option("fb_window_bits")},
           "proof_bytes_per_value": {"aggregate_16x16x16": pb / k, "u64_separate": 928},
           "ms_per_call": {name: {"median": statistics.median(v), "min": min(v), "max": max(v),
                                  "spread": (max(v) - min(v)) / statistics.median(v), "passes": v} for name, v in times.items()}}
    res["values_per_s"] = {name: m / (res["ms_per_call"][name]["median"] * 1e-3) for name in paths}
    res["aggregate_over_u64_per_value"] = res["values_per_s"]["aggregate_16x16x16"] / res["values_per_s"]["u64_separate"]
    agg.enable_timing(True)
    agg.timings(reset=True)
    path_agg()
    kt = agg.timings(reset=True)
    agg.enable_timing(False)
    kernels = {kn: {"ms": v["total_ms"], "launches": v["launches"]} for kn, v in kt.items() if v["launches"]}
    collect = kernels["k_aprove_collect"]["ms"]
    chain = sum(v["ms"] for kn, v in kernels.items()) - collect          # (the rerun is not part of the chain)
    res["kernels_ms_one_call_timing_on"] = kernels
    res["chain_ms_timing_on"] = chain
    res["collect_share_of_chain"] = collect / chain
    res["stage_b_share_of_chain"] = kernels["k_aprove_stage_b"]["ms"] / chain
    res["collect_share_of_stage_b"] = collect / kernels["k_aprove_stage_b"]["ms"]
    agg.close()
    u64.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({key: res[key] for key in ("instances", "values", "values_per_s", "aggregate_over_u64_per_value", "chain_ms_timing_on",
                                                "collect_share_of_chain", "stage_b_share_of_chain", "collect_share_of_stage_b")}
                     | {"median_ms": {name: v["median"] for name, v in res["ms_per_call"].items()},
                        "spread": {name: v["spread"] for name, v in res["ms_per_call"].items()},
                        "kernels": kernels}))


if __name__ == "__main__":
    main()
