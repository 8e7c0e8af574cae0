"""Cost of the seeded provers' device draws (include/bppp.h: "Seeded provers") against the `rnd` forms, at 2^14 and 2^16 values:
  device-resident   prove_batch_device (draws uploaded beforehand)  vs  prove_batch_seeded_device (k_draw_scalars + the same prover)
  host buffers      prove_batch (x, s and 52 x 32 bytes of draws uploaded per proof)  vs  prove_batch_seeded (x and s only)
plus the draw kernel alone (draw_scalars_device, n x 52 scalars).  Prints one JSON line per size; with an output path also writes them.
usage: python tools/seeded_prove_probe.py [out.json] [log2 sizes ...]           (default sizes 14 16)
Run under `rocprofv3 --kernel-trace --stats -- python tools/seeded_prove_probe.py` to see k_draw_scalars in the kernel list."""
import json
import os
import sys
import time

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import numpy as np
import torch

import bench
from bp_pp_amd import U64RangeProofProtocol, draw_scalars, synth

SEED = bytes(range(32))
args = sys.argv[1:]
out_path = args.pop(0) if args and not args[0].isdigit() else None
sizes = [1 << int(a) for a in args] or [1 << 14, 1 << 16]
gens, g, gv, hv = bench.load_generators()
proto = U64RangeProofProtocol(g, gv, hv, device=0)


def best_ms(fn, reps, rounds=3):
    fn(); proto.synchronize()
    best = 1e9
    for _ in range(rounds):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        proto.synchronize()
        best = min(best, (time.perf_counter() - t) / reps)
    return round(best * 1e3, 3)


rows = []
for n in sizes:
    x, s = synth.bulk_values(n), synth.bulk_blindings(n)
    rnd = draw_scalars(SEED, 0, n, 52).reshape(n, 52 * 32)
    dx, ds, dr = torch.from_numpy(x.view(np.int64)).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(rnd).cuda()
    oP = torch.zeros((n, 928), dtype=torch.uint8, device="cuda")
    oV = torch.zeros((n, 64), dtype=torch.uint8, device="cuda")
    oS = torch.zeros(n, dtype=torch.int32, device="cuda")
    dd = torch.zeros((n, 52, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    reps = max(3, min(20, (1 << 18) // n))
    r = {"n": n, "reps": reps}
    r["draw_kernel_ms"] = best_ms(lambda: proto.draw_scalars_device(SEED, 0, n, 52, dd.data_ptr()), reps)
    r["device_rnd_ms"] = best_ms(lambda: proto.prove_batch_device(synth.LABEL, n, dx.data_ptr(), ds.data_ptr(), dr.data_ptr(), oP.data_ptr(),
                                                                  oV.data_ptr(), oS.data_ptr()), reps)
    r["device_seeded_ms"] = best_ms(lambda: proto.prove_batch_seeded_device(synth.LABEL, n, dx.data_ptr(), ds.data_ptr(), SEED, 0,
                                                                            oP.data_ptr(), oV.data_ptr(), oS.data_ptr()), reps)
    r["host_rnd_ms"] = best_ms(lambda: proto.prove_batch(x, s, rnd, synth.LABEL), reps)
    r["host_seeded_ms"] = best_ms(lambda: proto.prove_batch_seeded(x, s, SEED, 0, synth.LABEL), reps)
    # the two forms agree (the same draws)
    p0, c0, _ = proto.prove_batch(x[:64], s[:64], rnd[:64], synth.LABEL)
    p1, c1, _ = proto.prove_batch_seeded(x[:64], s[:64], SEED, 0, synth.LABEL)
    r["agree"] = bool((p0 == p1).all() and (c0 == c1).all())
    r["draw_share_of_device_prove"] = round(r["draw_kernel_ms"] / r["device_rnd_ms"], 4)
    r["host_saving_ms"] = round(r["host_rnd_ms"] - r["host_seeded_ms"], 3)
    r["rnd_upload_mb"] = round(n * 52 * 32 / 1e6, 2)
    rows.append(r)
    print(json.dumps(r), flush=True)
proto.close()
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
