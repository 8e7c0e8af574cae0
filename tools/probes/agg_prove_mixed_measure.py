"""What PROVING aggregated range proofs of MIXED value counts in one call costs next to what a caller did before it: in ONE process on one
GPU, over ONE context of the (16, 16, 16) generators, 2^13 instances whose value counts k_i are drawn uniformly from 9 .. 16, draws made
on the device (the seeded device forms).

  1. "mixed_random"   bppp_reciprocal_agg_prove_values_batch_mixed_seeded_device, the instances in random order;
  2. "mixed_sorted"   the same instances sorted by k_i (a wavefront holds one value count, but for the class borders);
  3. "eight_uniform"  eight bppp_reciprocal_agg_prove_values_batch_seeded_device calls on that context, one per value count, on
                      per-class buffers gathered BEFORE the clock starts -- the gathering a caller has to do is not timed;
  4. "uniform_k16"    one uniform call on 2^13 instances of 16 values: what the padded fixed-base sums and the largest k_i cost anyway.

All are warmed up (every status checked, and the mixed outputs compared byte for byte with the per-class calls' on the same streams),
then `--passes` alternating passes of `--steps` calls each are timed with the host clock around calls that end in a stream synchronise;
per path the median pass and (max - min) / median.  One more call of each with per-kernel HIP events on gives the kernel table.  Then
paths 1 and 3 once more with "ct_prover" set (the full-scan table form of the secret-scalar sums), timed the same way in fewer passes.
Nothing here sets a target: it is the record of what was measured.

    python tools/probes/agg_prove_mixed_measure.py out.json [--lg-n 13] [--steps 2] [--passes 5]

Writes one JSON document to the path given; docs/design/07-prover-and-recip256.md section 7e has the table its numbers belong in."""
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
KS = list(range(9, 17))
LABEL = b"mixed aggregate prover probe"
SEED = bytes(range(32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lg-n", type=int, default=13)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--fb-window-bits", type=int, default=0)
    args = ap.parse_args()
    if torch.cuda.device_count() == 0:
        sys.exit("needs a GPU: nothing here is measured without one")
    import agg_cases as A
    from bp_pp_amd import _build, _capi
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol
    n, k_max, nd, np_ = 1 << args.lg_n, *SHAPE
    case = A.setup(*SHAPE)
    agg = AggregatedReciprocalRangeProofProtocol(*SHAPE, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0,
                                                 fb_window_bits=args.fb_window_bits)
    ctx, shape3 = agg._w._ctx, (case["rounds"], case["nl"], case["nn"])
    stride = case["proof_bytes"]
    pb = {k: A.proof_bytes(k, *shape3) for k in KS}
    rng = np.random.default_rng(20264)
    ks = rng.integers(KS[0], KS[-1] + 1, n).astype(np.uint8)
    x = np.zeros((n, k_max, 32), np.uint8)
    x[:, :, 24:] = rng.integers(0, 256, (n, k_max, 8), dtype=np.uint8)          # u64 values
    s = rng.integers(0, 256, (n, k_max, 32), dtype=np.uint8)
    s[:, :, 0] &= 0x7F
    uniform = _capi.symbol("bppp_reciprocal_agg_prove_values_batch_seeded_device")

    def inputs(order):
        """The instances in `order` (a permutation): device ks, x, s and outputs laid out by k_max."""
        return dict(ks=torch.from_numpy(np.ascontiguousarray(ks[order])).cuda(), x=torch.from_numpy(np.ascontiguousarray(x[order])).cuda(),
                    s=torch.from_numpy(np.ascontiguousarray(s[order])).cuda(), P=torch.zeros((n, stride), dtype=torch.uint8, device="cuda"),
                    C=torch.zeros((n, k_max, 64), dtype=torch.uint8, device="cuda"), st=torch.full((n,), 7, dtype=torch.int32, device="cuda"))

    ident, by_k = np.arange(n), np.argsort(ks, kind="stable")
    random_in, sorted_in = inputs(ident), inputs(by_k)
    # the per-class buffers of path 3: instance j of class k is row by_k[lo_k + j]; the mixed call on sorted_in gives it stream lo_k + j
    classes, lo = {}, 0
    for k in KS:
        rows = by_k[lo:lo + int((ks == k).sum())]
        m = len(rows)
        classes[k] = dict(lo=lo, m=m, x=torch.from_numpy(np.ascontiguousarray(x[rows, :k])).cuda(), s=torch.from_numpy(np.ascontiguousarray(s[rows, :k])).cuda(),
                          P=torch.zeros((m, pb[k]), dtype=torch.uint8, device="cuda"), C=torch.zeros((m, k, 64), dtype=torch.uint8, device="cuda"),
                          st=torch.full((m,), 7, dtype=torch.int32, device="cuda"))
        lo += m
    k16 = dict(x=random_in["x"], s=random_in["s"], P=torch.zeros((n, stride), dtype=torch.uint8, device="cuda"),
               C=torch.zeros((n, k_max, 64), dtype=torch.uint8, device="cuda"), st=torch.full((n,), 7, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()

    def mixed(inp):
        agg.prove_values_batch_mixed_seeded_device(LABEL, n, inp["ks"].data_ptr(), inp["x"].data_ptr(), inp["s"].data_ptr(), SEED, 0,
                                                   inp["P"].data_ptr(), inp["C"].data_ptr(), inp["st"].data_ptr())
        agg.synchronize()

    def eight_uniform():
        for k in KS:
            c = classes[k]
            _capi.check(uniform(ctx, LABEL, len(LABEL), c["m"], k, nd, np_, c["x"].data_ptr(), c["s"].data_ptr(), SEED, c["lo"], c["P"].data_ptr(),
                                c["C"].data_ptr(), c["st"].data_ptr()))
        agg.synchronize()

    def uniform_k16():
        _capi.check(uniform(ctx, LABEL, len(LABEL), n, k_max, nd, np_, k16["x"].data_ptr(), k16["s"].data_ptr(), SEED, 0, k16["P"].data_ptr(),
                            k16["C"].data_ptr(), k16["st"].data_ptr()))
        agg.synchronize()

    paths = {"mixed_random": lambda: mixed(random_in), "mixed_sorted": lambda: mixed(sorted_in), "eight_uniform": eight_uniform,
             "uniform_k16": uniform_k16}

    def check_outputs():
        """Every status zero; the sorted mixed call's rows equal the per-class calls' bytes (same inputs, same streams), zero behind them."""
        for inp in (random_in, sorted_in, k16, *classes.values()):
            assert not inp["st"].cpu().numpy().any()
        for k in KS:
            c = classes[k]
            rows = slice(c["lo"], c["lo"] + c["m"])
            assert torch.equal(sorted_in["P"][rows, :pb[k]], c["P"]) and not sorted_in["P"][rows, pb[k]:].any().item(), k
            assert torch.equal(sorted_in["C"][rows, :k], c["C"]) and not sorted_in["C"][rows, k:].any().item(), k

    for f in paths.values():
        f()
    check_outputs()

    def timed(names, passes):
        times = {name: [] for name in names}
        for _ in range(passes):
            for name in names:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    paths[name]()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
        return {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / statistics.median(v), "passes": v}
                for name, v in times.items()}

    def kernel_table(names):
        out = {}
        for name in names:
            agg.enable_timing(True)
            agg.timings(reset=True)
            paths[name]()
            kt = agg.timings(reset=True)
            agg.enable_timing(False)
            out[name] = {kn: {"ms": v["total_ms"], "launches": v["launches"]} for kn, v in kt.items() if v["launches"]}
        return out

    res = {"shape": list(SHAPE), "instances": n, "value_counts": {str(k): int((ks == k).sum()) for k in KS}, "values": int(ks.sum()),
           "steps": args.steps, "passes": args.passes, "device": torch.cuda.get_device_name(0), "device_code_sha256": _build.device_code_sha256(),
           "fb_window_bits": agg.get_option("fb_window_bits")}
    res["ms_per_call"] = timed(list(paths), args.passes)
    res["kernels_ms_one_call_timing_on"] = kernel_table(list(paths))
    agg.set_option("ct_prover", 1)
    ct_names = ["mixed_random", "eight_uniform"]
    for name in ct_names:
        paths[name]()                                                             # warm-up of the full-scan form; the same bytes
    check_outputs()
    res["ct_prover_ms_per_call"] = timed(ct_names, max(2, args.passes // 2))
    res["ct_prover_kernels_ms_one_call_timing_on"] = kernel_table(ct_names)
    agg.set_option("ct_prover", 0)
    med = {name: v["median"] for name, v in res["ms_per_call"].items()}
    res["mixed_random_over_eight_uniform"] = med["mixed_random"] / med["eight_uniform"]
    res["mixed_sorted_over_eight_uniform"] = med["mixed_sorted"] / med["eight_uniform"]
    res["mixed_random_over_uniform_k16"] = med["mixed_random"] / med["uniform_k16"]
    agg.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"median_ms": med, "ct_median_ms": {k: v["median"] for k, v in res["ct_prover_ms_per_call"].items()},
                      "kernels": res["kernels_ms_one_call_timing_on"], "ct_kernels": res["ct_prover_kernels_ms_one_call_timing_on"]}))


if __name__ == "__main__":
    main()
