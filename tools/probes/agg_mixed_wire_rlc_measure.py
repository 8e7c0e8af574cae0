"""What the wire (SEC1) form and the RLC mode of the mixed-value-count aggregate verifier cost: in ONE process on one GPU, over ONE
context of the (16, 16, 16) generators, 2^15 instances whose value counts k_i are drawn uniformly from 9 .. 16, in random order (the
method of tools/probes/agg_mixed_measure.py).  The proofs are made on the device by the seeded prover, one uniform call per value
count, every one accepted; the 33-byte slots are packed from them on the host before the clock starts.

  "mixed_exact"        bppp_reciprocal_agg_verify_batch_mixed_device (64-byte slots);
  "mixed_sec1"         ..._mixed_sec1_device: k_wire_expand_mixed in front of the same chain;
  "mixed_rlc"          ..._mixed_rlc_device, every proof valid;
  "mixed_rlc_1_in_1024" the same with one proof in 1,024 corrupted (a scalar of n);
  "mixed_rlc_sec1"     ..._mixed_rlc_sec1_device;
  "uniform_k16_sec1", "uniform_k16_rlc"  the uniform calls on 2^15 instances of 16 values, for scale (and "uniform_k16_exact").

All are warmed up (and every verdict checked), then `--passes` alternating passes of `--steps` calls each are timed with the host
clock around calls that end in a stream synchronise; per path the median pass and (max - min) / median.  The expansion's own cost is
reported as the difference of the medians of the wire call and its 64-byte twin, for the mixed and for the uniform k = 16 batch, and
for the mixed kernel also as the stand-alone launch of tests/emul/build_wire_mixed.py's runner (launch and synchronise included).
Nothing here sets a target: it is the record of what was measured.

    python tools/probes/agg_mixed_wire_rlc_measure.py out.json [--lg-n 15] [--steps 3] [--passes 5]

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
SEED = bytes(range(100, 132))


def pack_points(a64):
    """[..., 64] canonical points -> [..., 33] SEC1 (the identity: 33 zero bytes), as bp_pp_amd.wire.compress_point."""
    out = np.zeros(a64.shape[:-1] + (33,), np.uint8)
    out[..., 0] = np.where(a64.any(axis=-1), 2 + (a64[..., 63] & 1), 0)
    out[..., 1:] = a64[..., :32]
    return out


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
    from bp_pp_amd import _build, _capi, wire
    from bp_pp_amd.wnla import AggregatedReciprocalRangeProofProtocol
    from emul.build_wire_mixed import load as load_runner
    n, k_max, nd, np_ = 1 << args.lg_n, *SHAPE
    case = A.setup(*SHAPE)
    agg = AggregatedReciprocalRangeProofProtocol(*SHAPE, case["g"], case["gv"], case["hv"], case["gv_"], case["hv_"], device=0)
    ctx, shape3 = agg._w._ctx, (case["rounds"], case["nl"], case["nn"])
    rounds, S = case["rounds"], case["nl"] + case["nn"]
    stride, stride33 = case["proof_bytes"], agg.proof_sec1_bytes(*shape3)
    rng = np.random.default_rng(20263)
    ks = rng.integers(KS[0], KS[-1] + 1, n).astype(np.uint8)
    prove = _capi.symbol("bppp_reciprocal_agg_prove_values_batch_seeded_device")

    def made(k, m, stream_base):
        """m instances of k values from the seeded device prover: (proofs [m, pb(k)], commitments [m, k, 64]) on the host."""
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
        return dP.cpu().numpy(), dV.cpu().numpy()

    def packed(k, P64, V64):
        """-> (proofs33 [m, S(k)], commitments33 [m, k, 33])"""
        P = 4 + 2 * rounds + k
        m = P64.shape[0]
        q = np.concatenate([pack_points(P64[:, :64 * P].reshape(m, P, 64)).reshape(m, -1), P64[:, 64 * P:]], axis=1)
        assert q[0].tobytes() == wire.pack(P64[:1], P, S)[0].tobytes()
        return q, pack_points(V64)

    Q = np.zeros((n, stride), np.uint8)
    C = np.zeros((n, k_max, 64), np.uint8)
    Q33 = np.zeros((n, stride33), np.uint8)
    C33 = np.zeros((n, k_max, 33), np.uint8)
    base = 0
    for k in KS:
        rows = np.flatnonzero(ks == k)
        P64, V64 = made(k, len(rows), base)
        base += len(rows)
        q33, v33 = packed(k, P64, V64)
        Q[rows, :P64.shape[1]], C[rows, :k] = P64, V64
        Q33[rows, :q33.shape[1]], C33[rows, :k] = q33, v33
    P16, V16 = made(k_max, n, base)
    P16_33, V16_33 = packed(k_max, P16, V16)
    bad_rows = np.arange(517, n, 1024)
    Qbad = Q.copy()
    for r in bad_rows:                                     # the last scalar of the row's own proof: well-formed and wrong
        Qbad[r, A.proof_bytes(int(ks[r]), *shape3) - 32 + 17] ^= 0x10
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dK, dQ, dC, dQ33, dC33, dQbad = up(ks), up(Q), up(C), up(Q33), up(C33), up(Qbad)
    dP16, dV16, dP16_33, dV16_33 = up(P16), up(V16), up(P16_33), up(V16_33)
    dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dS = torch.zeros(n, dtype=torch.int32, device="cuda")
    dR = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    out = (dA.data_ptr(), dS.data_ptr())
    rej = dR.data_ptr()

    def mixed(method, q, c, seed=None):
        tail = () if seed is None else (seed,)
        getattr(agg, method)(LABEL, n, dK.data_ptr(), c.data_ptr(), q.data_ptr(), *shape3, *out, *tail, rej)
        agg.synchronize()

    def uniform(method, q, c, seed=None):
        tail = () if seed is None else (seed,)
        getattr(agg, method)(LABEL, n, c.data_ptr(), q.data_ptr(), *shape3, *out, *tail, rej)
        agg.synchronize()

    paths = {"mixed_exact": lambda: mixed("verify_batch_mixed_device", dQ, dC),
             "mixed_sec1": lambda: mixed("verify_batch_mixed_sec1_device", dQ33, dC33),
             "mixed_rlc": lambda: mixed("verify_batch_mixed_rlc_device", dQ, dC, SEED),
             "mixed_rlc_1_in_1024": lambda: mixed("verify_batch_mixed_rlc_device", dQbad, dC, SEED),
             "mixed_rlc_sec1": lambda: mixed("verify_batch_mixed_rlc_sec1_device", dQ33, dC33, SEED),
             "uniform_k16_exact": lambda: uniform("verify_batch_device", dP16, dV16),
             "uniform_k16_sec1": lambda: uniform("verify_batch_sec1_device", dP16_33, dV16_33),
             "uniform_k16_rlc": lambda: uniform("verify_batch_rlc_device", dP16, dV16, SEED)}
    rlc_used = {}
    for name, f in paths.items():            # warm-up, and every verdict checked
        dA.zero_()
        dS.fill_(7)
        f()
        acc, st = dA.cpu().numpy(), dS.cpu().numpy()
        want = np.ones(n, np.uint8)
        if name == "mixed_rlc_1_in_1024":
            want[bad_rows] = 0
        assert (acc == want).all() and not st.any() and int(dR.cpu()[0]) == int((want == 0).sum()), name
        if "rlc" in name:
            rlc_used[name] = [agg.get_option("last_rlc_superchunk"), agg.get_option("last_rlc_chunk")]
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
    # the mixed expansion kernel alone, through the test-only runner on the null stream (launch + device synchronise in the time)
    runner = load_runner("gfx950")
    dQ64 = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
    dC64 = torch.zeros((n, k_max, 64), dtype=torch.uint8, device="cuda")
    alone = []
    for i in range(1 + args.passes * args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = runner.wire_mixed_run_device(dC33.data_ptr(), dQ33.data_ptr(), dC64.data_ptr(), dQ64.data_ptr(), dK.data_ptr(), n, k_max, rounds, S)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0
        if i:
            alone.append(dt)
    used = np.zeros((n, stride), bool)
    for k in KS:
        used[ks == k, :A.proof_bytes(k, *shape3)] = True
    assert (dQ64.cpu().numpy()[used] == Q[used]).all()
    point_lanes = n * (k_max + 4 + 2 * rounds + k_max)
    idle = int(2 * (k_max - ks.astype(np.int64)).sum())
    res = {"shape": list(SHAPE), "instances": n, "value_counts": {str(k): int((ks == k).sum()) for k in KS}, "values": int(ks.sum()),
           "steps": args.steps, "passes": args.passes, "device": torch.cuda.get_device_name(0),
           "device_code_sha256": _build.device_code_sha256(), "fb_window_bits": agg.get_option("fb_window_bits"),
           "corrupted_rows": len(bad_rows), "last_rlc_superchunk_chunk": rlc_used,
           "ms_per_call": {name: {"median": med[name], "min": min(v), "max": max(v), "spread": (max(v) - min(v)) / med[name], "passes": v}
                           for name, v in times.items()},
           "expansion_ms": {"mixed_sec1_minus_exact": med["mixed_sec1"] - med["mixed_exact"],
                            "uniform_k16_sec1_minus_exact": med["uniform_k16_sec1"] - med["uniform_k16_exact"],
                            "k_wire_expand_mixed_alone": {"median": statistics.median(alone), "min": min(alone), "max": max(alone)}},
           "point_lanes": point_lanes, "idle_point_lanes": idle, "idle_point_lane_share": idle / point_lanes,
           "mixed_rlc_over_exact": med["mixed_rlc"] / med["mixed_exact"], "uniform_k16_rlc_over_exact": med["uniform_k16_rlc"] / med["uniform_k16_exact"]}
    agg.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"median_ms": med, "spread": {name: v["spread"] for name, v in res["ms_per_call"].items()},
                      "expansion_ms": res["expansion_ms"], "idle_point_lane_share": res["idle_point_lane_share"], "rlc": rlc_used}))


if __name__ == "__main__":
    main()
