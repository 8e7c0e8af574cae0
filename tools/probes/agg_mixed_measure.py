"""What verifying aggregated range proofs of MIXED value counts in one call costs next to what a caller did before it: in ONE process on
one GPU, over ONE context of the (16, 16, 16) generators, 2^15 instances whose value counts k_i are drawn uniformly from 9 .. 16.
The proofs are made on the device by the seeded prover, one uniform call per value count, every one accepted.

  1. "mixed_random"   bppp_reciprocal_agg_verify_batch_mixed_device, the instances in random order (neighbouring lanes differ in k_i);
  2. "mixed_sorted"   the same instances sorted by k_i (a wavefront holds one value count, but for the class borders);
  3. "eight_uniform"  eight bppp_reciprocal_agg_verify_batch_device calls, one per value count, on per-class buffers gathered
                      BEFORE the clock starts -- the gathering a caller has to do is not timed, which favours this path;
  4. "uniform_k16"    one uniform call on 2^15 instances of 16 values: what the padded fixed-base half and the largest k_i cost anyway.

All are warmed up (and every verdict checked), then `--passes` alternating passes of `--steps` calls each are timed with the host
clock around calls that end in a stream synchronise; per path the median pass and (max - min) / median.  One more call of each with
per-kernel HIP events on gives the kernel table.  Nothing here sets a target: it is the record of what was measured.

    python tools/probes/agg_mixed_measure.py out.json [--lg-n 15] [--steps 3] [--passes 5]

Writes one JSON document to the path given; docs/design/07-prover-and-recip256.md section 7d has the table its numbers belong in."""
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
LABEL = b"mixed aggregate probe"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--lg-n", type=int, default=15)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--passes", type=int, default=5)
    args = ap.parse_args()
    if torch.cuda.device_count() == 0:
        sys.exit("needs a GPU: nothing here is measured without one")
    import agg_cases as A
    from bp_pp_amd import _build, _capi
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol
    n, k_max, nd, np_ = 1 << args.lg_n, *SHAPE
    case = A.setup(*SHAPE)
    agg = AggregatedReciprocalRangeProofProtocol(*SHAPE, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0)
    ctx, shape3 = agg._w._ctx, (case["rounds"], case["nl"], case["nn"])
    stride = case["proof_bytes"]
    pb = {k: A.proof_bytes(k, *shape3) for k in KS}
    rng = np.random.default_rng(20263)
    ks = rng.integers(KS[0], KS[-1] + 1, n).astype(np.uint8)
    prove = _capi.symbol("bppp_reciprocal_agg_prove_values_batch_seeded_device")
    verify = _capi.symbol("bppp_reciprocal_agg_verify_batch_device")

    def made(k, m, stream_base):
        """m instances of k values from the seeded device prover: (proofs [m, pb(k)], commitments [m, k, 64]) on the device."""
        x = np.zeros((m, k, 32), np.uint8)
        x[:, :, 24:] = rng.integers(0, 256, (m, k, 8), dtype=np.uint8)
        s = rng.integers(0, 256, (m, k, 32), dtype=np.uint8)
        s[:, :, 0] &= 0x7F
        dX, dSb = torch.from_numpy(x).cuda(), torch.from_numpy(s).cuda()
        dP = torch.zeros((m, A.proof_bytes(k, *shape3)), dtype=torch.uint8, device="cuda")
        dV = torch.zeros((m, k, 64), dtype=torch.uint8, device="cuda")
        dSt = torch.zeros(m, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        _capi.check(prove(ctx, LABEL, len(LABEL), m, k, nd, np_, dX.data_ptr(), dSb.data_ptr(), bytes(range(32)), stream_base, dP.data_ptr(),
                          dV.data_ptr(), dSt.data_ptr()))
        agg.synchronize()
        assert not dSt.cpu().numpy().any(), k
        return dP, dV

    # the per-class buffers (what path 3 verifies), then the same instances scattered into k_max slots in random and in sorted order
    classes, base = {}, 0
    for k in KS:
        m = int((ks == k).sum())
        classes[k] = made(k, m, base)
        base += m
    dP16, dV16 = made(k_max, n, base)

    def slots(order_ks):
        dQ = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
        dC = torch.zeros((n, k_max, 64), dtype=torch.uint8, device="cuda")
        for k in KS:
            rows = torch.from_numpy(np.flatnonzero(order_ks == k)).cuda()
            dQ[rows, :pb[k]] = classes[k][0]
            dC[rows, :k] = classes[k][1]
        return dQ, dC, torch.from_numpy(np.ascontiguousarray(order_ks)).cuda()

    ks_sorted = np.sort(ks)
    random_in, sorted_in = slots(ks), slots(ks_sorted)
    dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dS = torch.zeros(n, dtype=torch.int32, device="cuda")
    dR = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def mixed(inp):
        dQ, dC, dK = inp
        agg.verify_batch_mixed_device(LABEL, n, dK.data_ptr(), dC.data_ptr(), dQ.data_ptr(), *shape3, dA.data_ptr(), dS.data_ptr(), dR.data_ptr())
        agg.synchronize()

    def eight_uniform():
        lo = 0
        for k in KS:
            dP, dV = classes[k]
            m = dP.shape[0]
            _capi.check(verify(ctx, LABEL, len(LABEL), m, k, nd, np_, dV.data_ptr(), dP.data_ptr(), *shape3, dA.data_ptr() + lo,
                               dS.data_ptr() + 4 * lo, None))
            lo += m
        agg.synchronize()

    def uniform_k16():
        _capi.check(verify(ctx, LABEL, len(LABEL), n, k_max, nd, np_, dV16.data_ptr(), dP16.data_ptr(), *shape3, dA.data_ptr(), dS.data_ptr(),
                           dR.data_ptr()))
        agg.synchronize()

    paths = {"mixed_random": lambda: mixed(random_in), "mixed_sorted": lambda: mixed(sorted_in), "eight_uniform": eight_uniform,
             "uniform_k16": uniform_k16}
    forms = {}
    for name, f in paths.items():            # warm-up, and every instance accepted
        dA.zero_()
        dS.fill_(7)
        f()
        assert dA.cpu().numpy().all() and not dS.cpu().numpy().any(), name
        forms[name] = agg._w.generic_form()
    times = {name: [] for name in paths}
    for _ in range(args.passes):
        for name, f in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                f()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    med = {name: statistics.median(v) for name, v in times.items()}
    res = {"shape": list(SHAPE), "instances": n, "value_counts": {str(k): int((ks == k).sum()) for k in KS}, "values": int(ks.sum()),
           "steps": args.steps, "passes": args.passes, "device": torch.cuda.get_device_name(0),
           "device_code_sha256": _build.device_code_sha256(), "fb_window_bits": agg.get_option("fb_window_bits"), "forms_last_call": forms,
           "ms_per_call": {name: {"median": med[name], "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med[name], "passes": v}
                           for name, v in times.items()},
           "mixed_random_over_eight_uniform": med["mixed_random"] / med["eight_uniform"],
           "mixed_random_over_uniform_k16": med["mixed_random"] / med["uniform_k16"],
           "mixed_random_over_mixed_sorted": med["mixed_random"] / med["mixed_sorted"]}
    kernels = {}
    for name, f in paths.items():
        agg.enable_timing(True)
        agg.timings(reset=True)
        f()
        kt = agg.timings(reset=True)
        agg.enable_timing(False)
        kernels[name] = {kn: {"ms": v["total_ms"], "launches": v["launches"]} for kn, v in kt.items() if v["launches"]}
    res["kernels_ms_one_call_timing_on"] = kernels
    agg.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({key: res[key] for key in ("instances", "values", "mixed_random_over_eight_uniform", "mixed_random_over_uniform_k16",
                                              "mixed_random_over_mixed_sorted")}
                     | {"median_ms": med, "spread": {name: v["spread"] for name, v in res["ms_per_call"].items()}, "kernels": kernels}))


if __name__ == "__main__":
    main()
