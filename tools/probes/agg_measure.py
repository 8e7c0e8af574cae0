"""What an aggregated reciprocal range proof costs the verifier per VALUE next to separate u64 proofs: in ONE process on one GPU, over
one pair of contexts,

  1. 2^15 aggregated instances of (k, nd, np) = (16, 16, 16) -- 2^19 u64 values -- through bppp_reciprocal_agg_verify_batch_device.  The
     instances are the few oracle-made proofs of tests/golden/agg_cases.json repeated (the oracle takes ten seconds per proof), every
     one accepted;
  2. 16 x 2^15 = 2^19 u64 proofs (made on the device by the seeded prover) through bppp_u64_verify_batch_device.

Both are warmed up, then `--passes` alternating passes of `--steps` calls each are timed with the host clock around calls that end in
a stream synchronise; per path the median pass, the spread of its passes and VALUES per second.  One more call of each with per-kernel
HIP events on gives the kernel table.  Nothing here sets a target: it is the record of what was measured.

    python tools/probes/agg_measure.py out.json [--lg-n 15] [--steps 3] [--passes 5]

Writes one JSON document to the path given; docs/design/07-prover-and-recip256.md has the section its numbers belong in."""
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
U64_LABEL = b"aggregate probe u64"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lg-n", type=int, default=15)
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
    case, coms, proofs, _ = agg_golden.load(SHAPE)
    agg = AggregatedReciprocalRangeProofProtocol(*SHAPE, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0)
    g, gv, hv = workload.split_generators(workload.make_batch(1, first=0)[0])
    u64 = U64RangeProofProtocol(g, gv, hv, device=0)
    idx = np.arange(n) % len(proofs)
    dC, dQ = torch.from_numpy(np.ascontiguousarray(coms[idx])).cuda(), torch.from_numpy(np.ascontiguousarray(proofs[idx])).cuda()
    dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dS = torch.zeros(n, dtype=torch.int32, device="cuda")
    dR = torch.zeros(1, dtype=torch.int32, device="cuda")
    m = n * k
    rng = np.random.default_rng(20262)
    dX = torch.from_numpy(rng.integers(0, 1 << 63, m, dtype=np.uint64).view(np.int64)).cuda()
    s = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    s[:, 0] &= 0x7F
    dSb = torch.from_numpy(s).cuda()
    dUP = torch.zeros((m, 928), dtype=torch.uint8, device="cuda")
    dUC = torch.zeros((m, 64), dtype=torch.uint8, device="cuda")
    dUA = torch.zeros(m, dtype=torch.uint8, device="cuda")
    dUS = torch.zeros(m, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    u64.prove_batch_seeded_device(U64_LABEL, m, dX.data_ptr(), dSb.data_ptr(), bytes(range(32)), 0, dUP.data_ptr(), dUC.data_ptr(), dUS.data_ptr())
    u64.synchronize()
    assert not dUS.cpu().numpy().any()

    def path_agg():
        agg.verify_batch_device(case["label"], n, dC.data_ptr(), dQ.data_ptr(), case["rounds"], case["nl"], case["nn"], dA.data_ptr(),
                                dS.data_ptr(), dR.data_ptr())
        agg.synchronize()

    def path_u64():
        u64.verify_batch_device(U64_LABEL, m, dUC.data_ptr(), dUP.data_ptr(), dUA.data_ptr(), dUS.data_ptr())
        u64.synchronize()

    paths = {"aggregate_16x16x16": path_agg, "u64_separate": path_u64}
    for f in paths.values():                 # warm-up, and every instance of both accepted
        f()
    assert dA.cpu().numpy().all() and not dS.cpu().numpy().any() and int(dR.cpu()[0]) == 0
    assert dUA.cpu().numpy().all() and not dUS.cpu().numpy().any()
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
           "aggregate_form": agg._w.generic_form(), "u64_plan": u64.last_plan(),
           "fb_window_bits": {"aggregate": agg.get_option("fb_window_bits"), "u64": u64.get_option("fb_window_bits")},
           "proof_bytes_per_value": {"aggregate_16x16x16": case["proof_bytes"] / k, "u64_separate": 928},
           "ms_per_call": {name: {"median": statistics.median(v), "min": min(v), "max": max(v),
                                  "spread": (max(v) - min(v)) / statistics.median(v), "passes": v} for name, v in times.items()}}
    res["values_per_s"] = {name: m / (res["ms_per_call"][name]["median"] * 1e-3) for name in paths}
    res["aggregate_over_u64_per_value"] = res["values_per_s"]["aggregate_16x16x16"] / res["values_per_s"]["u64_separate"]
    kernels = {}
    for name, (proto, f) in {"aggregate_16x16x16": (agg, path_agg), "u64_separate": (u64, path_u64)}.items():
        proto.enable_timing(True)
        proto.timings(reset=True)
        f()
        kt = proto.timings(reset=True)
        proto.enable_timing(False)
        kernels[name] = {kn: {"ms": v["total_ms"], "launches": v["launches"]} for kn, v in kt.items() if v["launches"]}
    res["kernels_ms_one_call_timing_on"] = kernels
    agg.close()
    u64.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({key: res[key] for key in ("instances", "values", "values_per_s", "aggregate_over_u64_per_value", "aggregate_form")}
                     | {"median_ms": {name: v["median"] for name, v in res["ms_per_call"].items()},
                        "spread": {name: v["spread"] for name, v in res["ms_per_call"].items()},
                        "kernels": kernels}))


if __name__ == "__main__":
    main()
