"""What the RLC mode buys the WNLA and circuit verifiers: times bppp_wnla_verify_batch[_rlc]_device at (16, 32) and
bppp_circuit_verify_batch[_rlc]_device at `mixed_k2`, 2^16 resident instances, all valid and with one instance in 1,024 corrupted, in
ONE process on one GPU: accept bits of every configuration checked first, every configuration warmed up, the settle time of
bench_other.two_passes, then `--passes` alternating passes of `--steps` calls each (host clock around calls that end in a stream
synchronise; the median pass is reported), then one pass per configuration with per-kernel HIP events on.  Batches are built as
bench_other.measure_wnla / measure_circuit build theirs.  --exact-only times the exact calls alone: for another build of the library
given through BPPP_LIB (the commit before the mode existed), to show that the exact path did not move.

    python tools/probes/generic_rlc_measure.py out.json
    BPPP_LIB=/path/to/earlier/libbppp_hip.so python tools/probes/generic_rlc_measure.py out_before.json --exact-only

Writes one JSON document to the path given; docs/design/09-rlc-and-bucket-stage.md has the section its numbers belong in."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import numpy as np
import torch

import bench_other
from bp_pp_amd import _capi, derive_generators, synth
from bp_pp_amd.wnla import ArithmeticCircuit, WeightNormLinearArgument

SEED = bytes(range(32))
SLICE = bench_other.GENERIC_SLICE


def build_wnla(total, ng=16, nh=32):
    label = b"wnla test"
    raw = derive_generators(b"bppp-bench-wnla", 1 + ng + nh)
    pts = [raw[64 * i:64 * i + 64] for i in range(1 + ng + nh)]
    w = WeightNormLinearArgument(pts[0], pts[1:1 + ng], pts[1 + ng:], device=0, fb_window_bits=0)
    bufs = {k: [] for k in ("com", "c", "rho", "mu", "pr", "px", "pl", "pn")}
    for a in range(0, total, SLICE):
        m = min(SLICE, total - a)
        sc = synth._bulk_scalars(b"wnla", a, m, nh + 1 + nh + ng, b"bppp-bench-wnla").reshape(m, -1, 32)
        c, rho, l, n = sc[:, :nh], sc[:, nh], sc[:, nh + 1:2 * nh + 1], sc[:, 2 * nh + 1:]
        rho_i = [int.from_bytes(bytes(r), "big") for r in rho]
        mu = np.frombuffer(b"".join((r * r % synth.N_ORDER).to_bytes(32, "big") for r in rho_i), np.uint8).reshape(m, 32)
        com, cst = w.commit_batch(c, mu, l, n)
        pr, px, pl, pn, pst = w.prove_batch(label, com, c, rho, mu, l, n)
        assert not cst.any() and not pst.any()
        for k, v in (("com", com), ("c", c), ("rho", rho), ("mu", mu), ("pr", pr), ("px", px), ("pl", pl), ("pn", pn)):
            bufs[k].append(np.ascontiguousarray(v))
    H = {k: np.concatenate(v) for k, v in bufs.items()}
    rounds, nl, nn = H["pr"].shape[1], H["pl"].shape[1], H["pn"].shape[1]
    D = {k: torch.from_numpy(v).cuda() for k, v in H.items()}
    bad = np.arange(0, total, 1024)
    Hbad = H["pn"].copy()
    Hbad[bad, 0, 31] ^= 1
    Dbad = dict(D, pn=torch.from_numpy(Hbad).cuda())
    dA = torch.zeros(total, dtype=torch.uint8, device="cuda")
    dS = torch.zeros(total, dtype=torch.int32, device="cuda")

    def call(d, rlc):
        args = (label, total, d["com"].data_ptr(), d["c"].data_ptr(), d["rho"].data_ptr(), d["mu"].data_ptr(), rounds, d["pr"].data_ptr(),
                d["px"].data_ptr(), d["pl"].data_ptr(), nl, d["pn"].data_ptr(), nn, dA.data_ptr(), dS.data_ptr())
        if rlc:
            w.verify_batch_rlc_device(*args, SEED)
        else:
            w.verify_batch_device(*args)

    return w, w, call, D, Dbad, bad, dA, dS


def build_circuit(total, name="mixed_k2"):
    with open(os.path.join(ROOT, "tests", "golden", "statements_generic.json")) as f:
        st = {c["name"]: c for c in json.load(f)["circuits"]}[name]
    nm, no, nv, k = st["dim_nm"], st["dim_no"], st["dim_nv"], st["k"]
    p2 = lambda x: 1 << max(0, (x - 1).bit_length())
    NG, NH = p2(nm), p2(nv + 9)
    raw = derive_generators(b"bppp-bench-circuit-" + name.encode(), 1 + NG + NH)
    pts = [raw[64 * i:64 * i + 64] for i in range(1 + NG + NH)]
    flat = lambda rows: np.frombuffer(b"".join(bytes.fromhex(x) for row in rows for x in row), np.uint8).reshape(-1, 32)
    vec = lambda xs: np.frombuffer(b"".join(bytes.fromhex(x) for x in xs), np.uint8).reshape(-1, 32)
    part = st["partition"]
    label = bytes.fromhex(st["label"])
    ac = ArithmeticCircuit(nm, no, k, nv, pts[0], pts[1:1 + nm], pts[1 + NG:1 + NG + nv + 9], flat(st["W_m"]), flat(st["W_l"]), vec(st["a_m"]),
                           vec(st["a_l"]), st["f_l"], st["f_m"], pts[1 + nm:1 + NG], pts[1 + NG + nv + 9:],
                           lambda typ, j: (None if part[typ][j] < 0 else part[typ][j]), device=0, fb_window_bits=0)
    v_one = np.stack([vec(row) for row in st["v"]])
    used = 18 + nv + nm
    coms, proofs, shape = [], [], None
    for a in range(0, total, SLICE):
        m = min(SLICE, total - a)
        sc = synth._bulk_scalars(b"circ", a, m, k + used, b"bppp-bench-circuit").reshape(m, -1, 32)
        s_v, rnd = sc[:, :k], sc[:, k:]
        v = np.broadcast_to(v_one, (m, k, nv, 32)).copy()
        com = np.stack([ac.commit_batch(v[:, j], s_v[:, j])[0] for j in range(k)], axis=1)
        rep = lambda xs: np.broadcast_to(vec(xs), (m,) + vec(xs).shape).copy()
        pr, pst, shape = ac.prove_batch(label, com, v, s_v, rep(st["w_l"]), rep(st["w_r"]), rep(st["w_o"]), rnd)
        assert not pst.any()
        coms.append(com); proofs.append(pr)
    Hc, Hp = np.concatenate(coms), np.concatenate(proofs)
    rounds, nl, nn = shape
    bad = np.arange(0, total, 1024)
    Hbad = Hp.copy()
    Hbad[bad, -1] ^= 1
    D = {"com": torch.from_numpy(Hc).cuda(), "p": torch.from_numpy(Hp).cuda()}
    Dbad = dict(D, p=torch.from_numpy(Hbad).cuda())
    dA = torch.zeros(total, dtype=torch.uint8, device="cuda")
    dS = torch.zeros(total, dtype=torch.int32, device="cuda")

    def call(d, rlc):
        args = (label, total, d["com"].data_ptr(), d["p"].data_ptr(), rounds, nl, nn, dA.data_ptr(), dS.data_ptr())
        if rlc:
            ac.verify_batch_rlc_device(*args, SEED)
        else:
            ac.verify_batch_device(*args)

    return ac, ac._w, call, D, Dbad, bad, dA, dS


def measure(name, built, total, steps, passes, exact_only):
    v, w, call, D, Dbad, bad, dA, dS = built
    stream = torch.cuda.Stream()
    _capi.check(_capi.lib().bppp_ctx_set_stream(w._ctx, stream.cuda_stream))
    torch.cuda.synchronize()

    def fence():
        v.synchronize()
        torch.cuda.synchronize()

    configs = [("exact_valid", D, False), ("exact_1in1024", Dbad, False)]
    if not exact_only:
        configs += [("rlc_valid", D, True), ("rlc_1in1024", Dbad, True)]
    out = {"total": total, "steps_per_pass": steps, "passes": passes, "ms": {k: [] for k, _, _ in configs}, "kernels_ms_per_call": {}}
    # results first: accept bits of every configuration
    for key, d, rlc in configs:
        dA.fill_(9); dS.fill_(7)
        call(d, rlc)
        fence()
        acc, st = dA.cpu().numpy(), dS.cpu().numpy()
        expect = np.ones(total, np.uint8)
        if d is Dbad:
            expect[bad] = 0
        assert (acc == expect).all() and not st.any(), key
    out["accept_bits_ok"] = True
    if not exact_only:
        out["rlc_used"] = {"superchunk": w.get_option("last_rlc_superchunk"), "chunk": w.get_option("last_rlc_chunk")}
    out["generic_form"] = w.generic_form()
    out["fb_window_bits"] = w.get_option("fb_window_bits")
    # warm-up of every configuration, then the settle time bench_other.two_passes uses, then alternating passes
    for key, d, rlc in configs:
        call(d, rlc)
    fence()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:
        call(D, False)
        fence()
    for _ in range(passes):
        for key, d, rlc in configs:
            fence()
            t0 = time.perf_counter()
            for _ in range(steps):
                call(d, rlc)
            fence()
            out["ms"][key].append((time.perf_counter() - t0) / steps * 1e3)
    # per-kernel times, a pass of their own with HIP events on
    for key, d, rlc in configs:
        v.enable_timing(True)
        v.timings(reset=True)
        for _ in range(steps):
            call(d, rlc)
        fence()
        kt = v.timings(reset=True)
        v.enable_timing(False)
        out["kernels_ms_per_call"][key] = {k: round(t["total_ms"] / steps, 4) for k, t in kt.items() if t["launches"]}
    out["median_ms"] = {k: float(np.median(x)) for k, x in out["ms"].items()}
    print(name, json.dumps(out["median_ms"]), flush=True)
    v.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--exact-only", action="store_true")
    ap.add_argument("--log2", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    total = 1 << a.log2
    doc = {"lib": os.environ.get("BPPP_LIB", "in-tree")}
    doc["wnla_16_32"] = measure("wnla_16_32", build_wnla(total), total, a.steps, a.passes, a.exact_only)
    doc["circuit_mixed_k2"] = measure("circuit_mixed_k2", build_circuit(total), total, a.steps, a.passes, a.exact_only)
    doc["device"] = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
