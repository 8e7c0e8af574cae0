"""What an aggregated reciprocal range proof costs the verifier per VALUE next to separate u64 proofs: in ONE process on one GPU, over
one pair of contexts,

  1. 2^15 aggregated instances of (k, nd, np) = (16, 16, 16) -- 2^19 u64 values -- through bppp_reciprocal_agg_verify_batch_device.  The
     instances are the few oracle-made proofs of tests/golden/agg_cases.json repeated (the oracle takes ten seconds per proof), every
     one accepted;
  2. 16 x 2^15 = 2^19 u64 proofs (made on the device by the seeded prover) through bppp_u64_verify_batch_device.

Beside the exact aggregate call, three more paths over the same instances on the same context: the RLC mode with every instance valid
("aggregate_rlc"), the RLC mode with one instance in 1,024 corrupted ("aggregate_rlc_1_in_1024_bad": a flipped bit in the last proof
scalar, so those chunks fall through to the exact sums) and the exact call over the wire form ("aggregate_sec1": 33-byte points,
expanded on the device).  The expansion launch has no timing bracket of its own; its share of the SEC1 call is taken from the medians
of the two exact paths, (sec1 - exact) / sec1.

All are warmed up, then `--passes` alternating passes of `--steps` calls each are timed with the host clock around calls that end in
a stream synchronise; per path the median pass, the spread of its passes and VALUES per second.  One more call of each with per-kernel
HIP events on gives the kernel table (which kernels take the time in RLC mode is read there).  Nothing here sets a target: it is the record of what was measured.

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
    from bp_pp_amd import U64RangeProofProtocol, _build, wire
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
    shape3 = (case["rounds"], case["nl"], case["nn"])
    # one instance in 1,024 well-formed and wrong: a bit flipped in the last proof scalar (never its top byte)
    bad = np.arange(512, n, 1024)
    Qbad = np.ascontiguousarray(proofs[idx])
    Qbad[bad, Qbad.shape[1] - 32 + 17] ^= 0x10
    dQbad = torch.from_numpy(Qbad).cuda()
    # the wire form of the same instances: the pool packed once, then repeated
    n_pts = 4 + 2 * case["rounds"] + k
    coms33 = wire.pack(coms.reshape(len(coms), -1), k).reshape(len(coms), k, 33)
    proofs33 = wire.pack(proofs, n_pts, case["nl"] + case["nn"])
    dC33, dQ33 = torch.from_numpy(np.ascontiguousarray(coms33[idx])).cuda(), torch.from_numpy(np.ascontiguousarray(proofs33[idx])).cuda()
    seed = bytes(range(100, 132))
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

    def path_rlc():
        agg.verify_batch_rlc_device(case["label"], n, dC.data_ptr(), dQ.data_ptr(), *shape3, dA.data_ptr(), dS.data_ptr(), seed, dR.data_ptr())
        agg.synchronize()

    def path_rlc_bad():
        agg.verify_batch_rlc_device(case["label"], n, dC.data_ptr(), dQbad.data_ptr(), *shape3, dA.data_ptr(), dS.data_ptr(), seed, dR.data_ptr())
        agg.synchronize()

    def path_sec1():
        agg.verify_batch_sec1_device(case["label"], n, dC33.data_ptr(), dQ33.data_ptr(), *shape3, dA.data_ptr(), dS.data_ptr(), dR.data_ptr())
        agg.synchronize()

    def path_u64():
        u64.verify_batch_device(U64_LABEL, m, dUC.data_ptr(), dUP.data_ptr(), dUA.data_ptr(), dUS.data_ptr())
        u64.synchronize()

    agg_paths = {"aggregate_16x16x16": path_agg, "aggregate_rlc": path_rlc, "aggregate_rlc_1_in_1024_bad": path_rlc_bad,
                 "aggregate_sec1": path_sec1}
    paths = dict(agg_paths, u64_separate=path_u64)
    for name, f in paths.items():            # warm-up, and every verdict what it must be: all accepted but the corrupted instances
        dA.zero_()
        f()
        if name == "aggregate_rlc_1_in_1024_bad":
            acc = dA.cpu().numpy()
            assert int(dR.cpu()[0]) == len(bad) and not acc[bad].any() and int(acc.sum()) == n - len(bad) and not dS.cpu().numpy().any()
            rlc_used = {"superchunk": agg.get_option("last_rlc_superchunk"), "chunk": agg.get_option("last_rlc_chunk")}
        elif name != "u64_separate":
            assert dA.cpu().numpy().all() and not dS.cpu().numpy().any() and int(dR.cpu()[0]) == 0, name
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
           "proof_bytes_per_value": {"aggregate_16x16x16": case["proof_bytes"] / k, "aggregate_sec1": proofs33.shape[1] / k, "u64_separate": 928},
           "rlc_used": rlc_used, "corrupted_instances": len(bad),
           "ms_per_call": {name: {"median": statistics.median(v), "min": min(v), "max": max(v),
                                  "spread": (max(v) - min(v)) / statistics.median(v), "passes": v} for name, v in times.items()}}
    res["values_per_s"] = {name: m / (res["ms_per_call"][name]["median"] * 1e-3) for name in paths}
    res["aggregate_over_u64_per_value"] = res["values_per_s"]["aggregate_16x16x16"] / res["values_per_s"]["u64_separate"]
    med = {name: res["ms_per_call"][name]["median"] for name in paths}
    res["over_exact"] = {name: med[name] / med["aggregate_16x16x16"] for name in agg_paths}
    res["sec1_expansion_share_of_call"] = (med["aggregate_sec1"] - med["aggregate_16x16x16"]) / med["aggregate_sec1"]
    kernels = {}
    for name, (proto, f) in ({name: (agg, f) for name, f in agg_paths.items()} | {"u64_separate": (u64, path_u64)}).items():
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
    print(json.dumps({key: res[key] for key in ("instances", "values", "values_per_s", "aggregate_over_u64_per_value", "aggregate_form", "over_exact",
                                              "sec1_expansion_share_of_call", "rlc_used")}
                     | {"median_ms": {name: v["median"] for name, v in res["ms_per_call"].items()},
                        "spread": {name: v["spread"] for name, v in res["ms_per_call"].items()},
                        "kernels": kernels}))


if __name__ == "__main__":
    main()
