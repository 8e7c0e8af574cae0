"""What the RLC mode costs and buys over WIRE input: times, in ONE process on one GPU, the four resident forms of the u64 verifier
    exact_64    bppp_u64_verify_batch_device            rlc_64    bppp_u64_verify_batch_rlc_device
    exact_sec1  bppp_u64_verify_batch_sec1_device       rlc_sec1  bppp_u64_verify_batch_rlc_sec1_device
for 2^16 and 2^20 proofs, all valid and with one proof in 1,024 corrupted.  The proofs are bench.py's synthetic batch, made by the
product prover in both forms (the 928-byte and the 525-byte output of the same inputs); the accept bits of every configuration are
checked first, every configuration is warmed up, then `--passes` alternating passes of `--steps` calls each are timed (host clock around
calls that end in a stream synchronise; the median pass is reported).  The RLC forms run with the context's automatic choices
("rlc_superchunk", "rlc_chunk" from the previous call's reject rate), as a caller gets them.

    python tools/probes/rlc_sec1_measure.py out.json [--log2 16 20]

Writes one JSON document to the path given; docs/design/09-rlc-and-bucket-stage.md has the section its numbers belong in."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]

import numpy as np
import torch

from bp_pp_amd import U64RangeProofProtocol, _capi, synth

SEED = bytes(range(32))
SLICE = 1 << 16
FORMS = ("exact_64", "exact_sec1", "rlc_64", "rlc_sec1")


def load_generators():
    with open(os.path.join(ROOT, "tests", "golden", "u64_golden.json")) as f:
        gens = bytes.fromhex(json.load(f)["generators"])
    return gens[:64], [gens[64 * i:64 * i + 64] for i in range(1, 17)], [gens[64 * i:64 * i + 64] for i in range(17, 49)]


def build(proto, n):
    """n proofs resident in both forms, and a second copy of each proof array with one proof in 1,024 corrupted (a bit of a trailing
    scalar: the last 96 bytes of both forms)."""
    d64, d928 = torch.empty((n, 64), dtype=torch.uint8, device="cuda"), torch.empty((n, 928), dtype=torch.uint8, device="cuda")
    d33, d525 = torch.empty((n, 33), dtype=torch.uint8, device="cuda"), torch.empty((n, 525), dtype=torch.uint8, device="cuda")
    dSt = torch.zeros(n, dtype=torch.int32, device="cuda")
    for a in range(0, n, SLICE):
        b = min(n, a + SLICE)
        x = torch.from_numpy(synth.bulk_values(b - a, first=a).view(np.int64)).cuda()
        s = torch.from_numpy(synth.bulk_blindings(b - a, first=a)).cuda()
        r = torch.from_numpy(synth.bulk_prover_randomness(b - a, first=a)).cuda()
        torch.cuda.synchronize()
        proto.prove_batch_device(synth.LABEL, b - a, x.data_ptr(), s.data_ptr(), r.data_ptr(), d928[a:b].data_ptr(), d64[a:b].data_ptr(),
                                 dSt[a:b].data_ptr())
        proto.prove_batch_sec1_device(synth.LABEL, b - a, x.data_ptr(), s.data_ptr(), r.data_ptr(), d525[a:b].data_ptr(), d33[a:b].data_ptr(),
                                      dSt[a:b].data_ptr())
        proto.synchronize()
        del x, s, r
    assert not bool(dSt.any().item())
    bad = np.arange(0, n, 1024, dtype=np.int64)
    offs = np.array([synth.corrupt_offset(int(j)) for j in bad], dtype=np.int64)
    ti, to = torch.from_numpy(bad).cuda(), torch.from_numpy(offs).cuda()
    b928, b525 = d928.clone(), d525.clone()
    b928[ti, to] = b928[ti, to] ^ 1
    b525[ti, to - 832 + 429] = b525[ti, to - 832 + 429] ^ 1
    torch.cuda.synchronize()
    return {"valid": (d64, d928, d33, d525), "1in1024": (d64, b928, d33, b525)}, bad


def measure(proto, n, steps, passes):
    data, bad = build(proto, n)
    dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dS = torch.zeros(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    _capi.check(_capi.lib().bppp_ctx_set_stream(proto._ctx, stream.cuda_stream))
    torch.cuda.synchronize()

    def call(form, content):
        c64, p928, c33, p525 = data[content]
        if form == "exact_64":
            proto.verify_batch_device(synth.LABEL, n, c64.data_ptr(), p928.data_ptr(), dA.data_ptr(), dS.data_ptr(), 0, 0)
        elif form == "exact_sec1":
            proto.verify_batch_sec1_device(synth.LABEL, n, c33.data_ptr(), p525.data_ptr(), dA.data_ptr(), dS.data_ptr(), 0, 0)
        elif form == "rlc_64":
            proto.verify_batch_rlc_device(synth.LABEL, n, c64.data_ptr(), p928.data_ptr(), dA.data_ptr(), SEED, d_status=dS.data_ptr())
        else:
            proto.verify_batch_rlc_sec1_device(synth.LABEL, n, c33.data_ptr(), p525.data_ptr(), dA.data_ptr(), SEED, d_status=dS.data_ptr())

    def fence():
        proto.synchronize()
        torch.cuda.synchronize()

    configs = [(f, c) for c in ("valid", "1in1024") for f in FORMS]
    out = {"proofs": n, "steps_per_pass": steps, "passes": passes, "ms": {"%s/%s" % fc: [] for fc in configs}, "rlc_used": {}}
    for form, content in configs:                       # results first
        dA.fill_(9); dS.fill_(7)
        call(form, content)
        fence()
        expect = np.ones(n, np.uint8)
        if content == "1in1024":
            expect[bad] = 0
        assert (dA.cpu().numpy() == expect).all() and not bool(dS.any().item()), (form, content)
    out["accept_bits_ok"] = True
    for form, content in configs:                       # warm-up (twice: the RLC forms plan from the previous call's reject rate)
        call(form, content)
        call(form, content)
    fence()
    for _ in range(passes):
        for form, content in configs:
            proto.set_option("rlc_history", 0)
            if form.startswith("rlc"):                  # the plan a caller in this regime gets: one call of the same content before
                call(form, content)
            fence()
            t0 = time.perf_counter()
            for _ in range(steps):
                call(form, content)
            fence()
            out["ms"]["%s/%s" % (form, content)].append((time.perf_counter() - t0) / steps * 1e3)
            if form.startswith("rlc"):
                out["rlc_used"]["%s/%s" % (form, content)] = {"superchunk": proto.get_option("last_rlc_superchunk"),
                                                               "chunk": proto.get_option("last_rlc_chunk")}
    out["median_ms"] = {k: float(np.median(v)) for k, v in out["ms"].items()}
    out["verifies_per_s"] = {k: n / v * 1e3 for k, v in out["median_ms"].items()}
    print(n, json.dumps({k: round(v / 1e6, 3) for k, v in out["verifies_per_s"].items()}), "M/s", flush=True)
    _capi.check(_capi.lib().bppp_ctx_set_stream(proto._ctx, None))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--fb-window-bits", type=int, default=0)
    a = ap.parse_args()
    g, gv, hv = load_generators()
    proto = U64RangeProofProtocol(g, gv, hv, device=0, fb_window_bits=a.fb_window_bits)
    doc = {"device": torch.cuda.get_device_name(0), "fb_window_bits": proto.get_option("fb_window_bits"),
           "device_code_sha256": __import__("bp_pp_amd._build", fromlist=["x"]).device_code_sha256()}
    try:
        for lg in a.log2:
            doc["2pow%d" % lg] = measure(proto, 1 << lg, a.steps, a.passes)
    finally:
        proto.close()
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
