#!/usr/bin/env python3
"""bench.py -- u64 range-proof batch verification throughput on MI355X (BASELINE.json metric).

Default workload (BASELINE.json configs[2], the configuration `north_star` quotes the metric on): ONE fixed batch of 2^20
independent u64 range proofs that share one generator set, split contiguously by proof index over the N GPUs
(`shard_range`: 2^20 / N proofs per GPU; N = 1 keeps all 2^20 resident on one GPU) -- strong scaling.  One "step" = one pass
of the exact per-proof verify pipeline over the whole batch, inputs already resident in HBM, followed by the single
accept-reduce: one 4-byte all-reduce of the reject count over RCCL (a no-op at N = 1).  There is no data-path collective.

A plain run (`bench.py --gpus N --steps K --warmup W`) sets up, runs W untimed and K timed steps, checks the accept bits and the
reject count of the last step, and prints ONE JSON line on rank 0: metric, value, unit, ms_per_step (wall time of one timed step),
higher_is_better, dtype, config, accept_bits_ok, ranks, setup_s.  `--dump-outputs DIR` also writes what the last timed step
computed -- accept.npy, status.npy (per proof of the rank's shard) and reject_count.npy -- before the line is printed.

`--full` measures everything else on top, after the same timed steps, and adds it to the line:
  roofline     -- dominant kernel: algorithmic bytes per launch (559 B/verify, SURVEY.md 8d, x the proofs one launch
                  processes) / its average launch duration, measured with HIP events on the launch stream in a second pass
                  of the same steps (timing_pass, kernels_ms_per_step), against 8 TB/s; `traffic` = measured HBM bytes per
                  launch from the committed PMC passes; roofline_valu against tools/ratebench's issue rates, measured by the same run.
  cpu_baseline -- the reference-shaped C restatement (oracle/, kind "port": the Rust reference cannot be built here)
                  timed on this box's host cores on a bounded sample of the same workload (rank 0, N = 1 only).
Secondary objects (never `value`; --no-secondary leaves them out): configs[1] (2^16 proofs on one GPU), the shares of an
N-GPU split, the optional RLC batch mode, the host-buffer (PCIe-inclusive) entry point, the table sweep.

Other workloads, each printing its own JSON line with `roofline` and `cpu_baseline`:
  --workload prove     BASELINE configs[3]: batch-prove 2^14 u64 values on one GPU (2262 algorithmic B/prove)
  --workload recip256  BASELINE configs[4]: ONE fixed batch of 2^18 ReciprocalRangeProofProtocol (dim_nd 256, dim_np 16) proofs
                       split over the N GPUs like the headline metric (823 algorithmic B/verify)
  --workload wnla      the crate's generic `wnla::verify` (wnla.rs:75-121): 2^16 instances of N = 16 / 32, device-resident
  --workload circuit   the crate's generic `circuit::verify` (circuit.rs:154-256): 2^16 instances of --statement mixed_k2 | ac_works
Under --full the default line also carries reduced-size runs of prove, recip256, wnla and circuit as secondary objects
(`prove_2pow14`, `recip256_2pow15`, `wnla_16_32_2pow16`, `circuit_mixed_k2_2pow16`).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ALGO_BYTES_PER_VERIFY = 13 * 33 + 3 * 32 + 33 + 1   # 559 B: SEC1 proof + commitment + accept byte
ALGO_BYTES_PER_PROVE = 8 + 32 + 52 * 32 + 13 * 33 + 96 + 33   # 2262 B
ALGO_BYTES_PER_RECIP256 = 21 * 33 + 96 + 33 + 1     # 823 B
HBM_PEAK_GBS = 8000.0                               # MI355X_MICROARCH.md: 8.0 TB/s spec
# VALU issue ceilings for the 256-bit integer mix (G wave-instructions/s per chip):
#   datasheet: 1024 SIMDs x 2.4 GHz; a wave64 full-rate op issues in 2 cycles, v_mad_u64_u32 / 64-bit shifts in 4
#   measured : tools/ratebench (built by __graft_entry__.build()) run by THIS bench process on THIS box before the timed region:
#              lane-ops/s of v_mad_u64_u32 and of add/shift/xor at 8 waves per SIMD, with the shader clock the chip held meanwhile
DATASHEET_SIMD_HZ = 1024 * 2.4e9
_SESSION_RATES = None


def under_profiler():
    """rocprofv3 preloads its tool library into this process (and into any child it starts): no child processes then."""
    return "rocprof" in os.environ.get("LD_PRELOAD", "") or any(k.startswith(("ROCPROFILER_", "ROCPROF_", "ROCP_")) for k in os.environ)


def session_rates(measure=False):
    """Issue rates of this box (a child process: tools/ratebench, ~1 s).  Measured ONLY when main() asks for it -- at the very top,
    before this process has imported torch or made any HIP call, so the child is started from a process that has never touched the
    GPU -- and never under rocprofv3; every later call returns what was measured then.  None if the tool is missing, fails or was
    skipped: roofline_valu then reports the datasheet ceiling only; it never falls back to another session's numbers."""
    global _SESSION_RATES
    if _SESSION_RATES is None and not measure:
        _SESSION_RATES = {}
    if _SESSION_RATES is None:
        import subprocess
        exe = os.path.join(ROOT, "tools", "ratebench")
        try:
            out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
            _SESSION_RATES = json.loads(out.stdout) if out.returncode == 0 else {}
        except Exception:
            _SESSION_RATES = {}
    return _SESSION_RATES or None


_BUILD_ID = None


def build_id():
    """SHA-256 of the device code of the library this process loads (bp_pp_amd/_build.py: device_code_sha256)."""
    global _BUILD_ID
    if _BUILD_ID is None:
        from bp_pp_amd import _build
        _BUILD_ID = _build.device_code_sha256(os.environ.get("BPPP_LIB", _build.SO)) or "unknown"
    return _BUILD_ID


def pmc_file(name):
    """A committed PMC summary (profiles/pmc_traffic.json, profiles/pmc_valu.json) -- or None when it was collected on other kernels
    than the ones being timed: tools/pmc_summarize.py / tools/sq_summarize.py stamp the summaries with the device code's hash."""
    d = _load_json(os.path.join(ROOT, "profiles", name))
    if not d:
        return None
    have = d.get("code_object_sha256") or (d.get("_meta") or {}).get("code_object_sha256")
    return d if have == build_id() else None


def pmc_matches_build():
    return {"traffic": pmc_file("pmc_traffic.json") is not None, "valu": pmc_file("pmc_valu.json") is not None, "code_object_sha256": build_id()}


def _load_json(path):
    try:
        with open(path) as f:
            return json.load(f)
    except Exception:
        return None


def launched_kernel(kernel, n_proofs, lanes_per_proof):
    """The library's timing slots are per stage; from 2^17 proofs per launch the u64 verifier's two fixed-base stages run their
    one-lane-per-proof kernels (k_verify_*_l1), which is the name the rocprofv3 summaries carry."""
    if kernel in ("k_verify_c0_fixed", "k_verify_final_check") and n_proofs >= (1 << 17):
        return kernel + "_l1", 1
    if kernel == "k_prove_msm":        # the prover's sums: lanes per proof by batch size (bppp_u64.hip: PMSMX); the fused launches dominate
        if n_proofs >= (1 << 17):
            return "k_prove_msm_l1x", 1
        if n_proofs >= (1 << 14):
            return "k_prove_msm_l4x", 4
        return ("k_prove_msm_l64x", 64) if n_proofs <= 1024 else ("k_prove_msm_x", 8)
    return kernel, lanes_per_proof


def valu_roofline(kernel, avg_ms, n_proofs, lanes_per_proof):
    """Compute-side ceiling of one kernel: VALU wave-instructions per launch (SQ_INSTS_VALU per wave from the committed
    rocprofv3 --pmc pass, times the waves this launch ran) over the live-measured launch time, against the issue rate of the
    kernel's own instruction mix.  The mix -- the fraction of half-rate instructions (v_mad_u64_u32, 64-bit shifts / adds) -- is
    MEASURED per kernel: SQ_INSTS_VALU_INT64 / SQ_INSTS_VALU from the same PMC passes (profiles/pmc_valu.json), with the static
    count of the shipped code object (tools/isa_mix.py -> profiles/isa_mix.json) printed beside it as a cross-check.  Two peaks:
    datasheet (1024 SIMDs x 2.4 GHz, 2 cycles per full-rate and 4 per half-rate wave64 instruction) and this box's own
    micro-benchmark, run by this process (session_rates: tools/ratebench, which also reports the shader clock the chip held)."""
    pv = pmc_file("pmc_valu.json")
    if pv is None:
        return None          # no counters for THIS build: say nothing rather than quote another build's
    mix = _load_json(os.path.join(ROOT, "profiles", "isa_mix.json")) or {}
    kernel, lanes_per_proof = launched_kernel(kernel, n_proofs, lanes_per_proof)
    kv = pv.get(kernel, {})
    per_wave = kv.get("valu_insts_per_wave")
    half_static = (mix.get(kernel) or {}).get("half_rate_frac")
    half = kv.get("int64_frac_of_valu", half_static)
    if not per_wave or half is None:
        return None
    waves = (n_proofs * lanes_per_proof + 63) // 64
    insts = per_wave * waves
    ach = insts / (avg_ms * 1e-3) / 1e9
    peak_ds = DATASHEET_SIMD_HZ / (half * 4 + (1 - half) * 2) / 1e9
    rates = session_rates()
    peak_ms = None
    if rates:
        peak_ms = 1.0 / (half / (rates["mad_u64_u32"] / 64) + (1 - half) / (rates["add_xor_shift"] / 64)) / 1e9
    return {"kernel": kernel, "wave_insts_per_launch": insts, "achieved": ach, "unit": "G wave-instructions/s",
            "half_rate_inst_frac": half, "half_rate_inst_frac_source": "SQ_INSTS_VALU_INT64 / SQ_INSTS_VALU (rocprofv3 --pmc)" if "int64_frac_of_valu" in kv else "static ISA count",
            "half_rate_inst_frac_static_isa": half_static,
            "peak_datasheet": peak_ds, "frac_of_datasheet": ach / peak_ds,
            "peak_microbench": peak_ms, "frac_of_microbench": (ach / peak_ms) if peak_ms else None,
            "peak_microbench_session": dict(rates, source="tools/ratebench run by this bench process on this box, before the timed region") if rates else None,
            "valu_active_frac_of_wave_cycles": kv.get("SQ_ACTIVE_INST_VALU_frac_of_wave_cycles"),
            "issue_stall_frac_of_wave_cycles": kv.get("SQ_WAIT_INST_ANY_frac_of_wave_cycles"),
            "wait_frac_of_wave_cycles": kv.get("SQ_WAIT_ANY_frac_of_wave_cycles")}


def pmc_traffic(kernel, n_proofs):
    """Measured HBM bytes per launch of `kernel` (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, corrected
    as tools/pmc_summarize.py documents), scaled linearly if the committed pass ran a different batch size."""
    tr = pmc_file("pmc_traffic.json") or {}
    kernel = launched_kernel(kernel, n_proofs, 1)[0]
    k = (tr.get("kernels") or {}).get(kernel) or {}
    b = k.get("hbm_bytes_per_launch")
    if b is None:
        return None
    n_ref = k.get("proofs_per_launch") or tr.get("proofs_per_launch") or 65536
    return b * (n_proofs / n_ref)      # the PMC pass of this kernel ran n_ref proofs per launch


SHARED_INV = 0      # proofs per shared field inversion in the timed verify calls (the plan's shared_inv; set by main() from last_plan())


def shared_inv_of(plan_text):
    """`shared_inv=G` of a plan description (bppp_plan_describe); 0 when the library predates the field."""
    for tok in (plan_text or "").split():
        if tok.startswith("shared_inv="):
            return int(tok.split("=")[1])
    return 0


def slot_kernels(slot, launches_per_step):
    """The kernels behind one of the library's timing slots, with their launches per step: one kernel per slot, except where the
    plan shares field inversions (from 2^18 proofs) -- there the table build is five pass kernels and the inverting launches
    (+ the join of C0's halves ahead of round 1) have a slot of their own."""
    if SHARED_INV and slot == "k_verify_tables":
        return [("k_verify_tables_pass%d" % i, launches_per_step / 5.0) for i in range(5)]
    if slot == "k_verify_shared_inv":
        # eight timed launches per step, each one inverting kernel; the one ahead of round 1 also holds the join of C0's halves
        return [("k_verify_shared_inv%d" % SHARED_INV, launches_per_step), ("k_verify_c0_join", launches_per_step / 8.0)]
    return [(slot, launches_per_step)]


def pmc_traffic_per_step(kernel_times, steps, n_proofs):
    """Counter bytes of ALL kernels of one step (each kernel's measured bytes per launch x its launches per step), or None when a
    kernel of the step has no counters for this build."""
    total = 0.0
    for slot, v in kernel_times.items():
        if not v["launches"]:
            continue
        for k, per_step in slot_kernels(slot, v["launches"] / steps):
            b = pmc_traffic(k, n_proofs)
            if b is None:
                if k in ("k_verify_accept",):      # (a few bytes per proof; absent from some passes)
                    continue
                return None
            total += b * per_step
    return total


FB_KERNELS = ("k_verify_c0_fixed", "k_verify_final_check", "k_prove_msm", "k_wnla_msm", "k_recip_c0_fixed")


def setup_dist(args):
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # diagnostics for a one-GPU box: BENCH_ONE_DEVICE=1 maps every rank to device 0 and BENCH_DIST_BACKEND=gloo replaces RCCL (which
    # refuses two ranks on one device), so that `torch.distributed.run --nproc-per-node 2 bench.py --gpus 2` dry-runs the N > 1
    # logic (shards, barrier, reject-count reduce, max-over-ranks timing) on real kernels; never a measurement
    if os.environ.get("BENCH_ONE_DEVICE"):
        local_rank = 0
    backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")
    if args.gpus != world:
        # (python3 bench.py --gpus N without a launcher never gets here: main() starts the ranks itself -- launch_ranks)
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: start one rank per GPU (torch.distributed.run --nproc-per-node {args.gpus}), "
              "or run plain `python3 bench.py --gpus N`, which does that itself", file=sys.stderr)
        sys.exit(2)
    if not torch.cuda.is_available():
        print("bench.py: no GPU visible; the bp_pp_amd product path has no CPU fallback", file=sys.stderr)
        sys.exit(3)
    torch.cuda.set_device(local_rank)
    # BENCH_FORCE_DIST=1: initialise RCCL even for one rank, so that the N > 1 code path (process group, barrier, the reject-count
    # all-reduce on the verify stream) can be exercised on a one-GPU box
    if world > 1 or os.environ.get("BENCH_FORCE_DIST"):
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank), rank=rank, world_size=world)
        else:
            dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return world, rank, local_rank


def launch_ranks(n_ranks):
    """`python3 bench.py --gpus N` with no launcher around it: start the N ranks as CHILD processes under torch.distributed.run (what
    the driver's SCALE command spells out itself), relay what they print and their exit code.  Called before this process has imported
    torch or made any HIP call -- a process that has touched the GPU must never replace its image, and this one does not even exec: the
    launcher is a child.  Not possible under rocprofv3 (its preloaded tool library would follow into the children)."""
    import socket
    import subprocess
    if under_profiler():
        print("bench.py: --gpus N > 1 under rocprofv3: profile one rank (--gpus 1 --total-proofs <share>) instead", file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: what RCCL across processes needs on this image
    env["BENCH_SELF_LAUNCHED"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_ranks}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def predicted_scaling(total, ms_one_gpu, shares):
    """What N GPUs would do with the SAME batch, from one GPU's measured time on its share (the shares run on this box, on the shipping
    plan; shard_range is contiguous and the proofs are i.i.d., so rank 0's share stands for every rank's).  Not a measurement of N GPUs:
    the 4-byte RCCL all-reduce of the reject count (one latency, tens of microseconds) and rank skew are not in it."""
    out = {"1": {"share": total, "ms_per_step": ms_one_gpu, "value": total / ms_one_gpu * 1e3, "efficiency": 1.0}}
    for lg, sh in sorted(shares.items(), reverse=True):
        n_gpus = total >> lg
        if n_gpus < 2 or (total >> lg) << lg != total:
            continue
        v = total / sh["ms_per_step"] * 1e3
        out[str(n_gpus)] = {"share": 1 << lg, "ms_per_step": sh["ms_per_step"], "value": v, "efficiency": v / (n_gpus * out["1"]["value"])}
    out["note"] = ("derived from ONE GPU: total proofs / the time this GPU takes for a 1/N share; excludes the 4-byte reject-count all-reduce and "
                   "rank skew; no N > 1 hardware run exists in this pool")
    return out


def measure_sec1_device(torch, proto, workload, n, expect, steps, stream, slice_proofs=1 << 16):
    import numpy as np
    d33 = torch.empty((n, 33), dtype=torch.uint8, device="cuda")
    d525 = torch.empty((n, 525), dtype=torch.uint8, device="cuda")
    dSt = torch.zeros(n, dtype=torch.int32, device="cuda")
    for a in range(0, n, slice_proofs):
        b = min(n, a + slice_proofs)
        x = torch.from_numpy(workload.bulk_values(b - a, first=a).view(np.int64)).cuda()
        s = torch.from_numpy(workload.bulk_blindings(b - a, first=a)).cuda()
        r = torch.from_numpy(workload.bulk_prover_randomness(b - a, first=a)).cuda()
        torch.cuda.synchronize()
        proto.prove_batch_sec1_device(workload.LABEL, b - a, x.data_ptr(), s.data_ptr(), r.data_ptr(), d525[a:b].data_ptr(), d33[a:b].data_ptr(), dSt[a:b].data_ptr())
        proto.synchronize()
        del x, s, r
    # the same proofs as the headline batch, so the same ones are corrupted: one bit of a trailing scalar (the scalars are the last 96 bytes
    # of both forms: offset in the 928-byte form - 832 + 429)
    bad = np.nonzero(expect == 0)[0]
    if len(bad):
        ti = torch.from_numpy(bad).cuda()
        to = torch.from_numpy(np.array([workload.corrupt_offset(int(j)) - 832 + 429 for j in bad], dtype=np.int64)).cuda()
        d525[ti, to] = d525[ti, to] ^ 1
    dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dS = torch.zeros(n, dtype=torch.int32, device="cuda")

    def step():
        with torch.cuda.stream(stream):
            proto.verify_batch_sec1_device(workload.LABEL, n, d33.data_ptr(), d525.data_ptr(), dA.data_ptr(), dS.data_ptr(), 0, 0)
    step(); step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    ok = bool((dA.cpu().numpy() == expect).all()) and not bool(dS.any().item()) and not bool(dSt.any().item())
    return {"value": n / ms * 1e3, "unit": "verifies/s", "ms_per_step": ms, "proofs": n, "accept_bits_ok": ok,
            "bytes_per_proof_read": 525 + 33, "algorithmic_bytes_per_proof": ALGO_BYTES_PER_VERIFY,
            "note": "bppp_u64_verify_batch_sec1_device on the whole batch in the reference's wire form, resident in HBM (what the device reads per "
                    "proof IS the 559 algorithmic bytes less the accept byte); the same proofs and the same corrupted ones as the headline batch; "
                    "kernel timing off; never `value`"}


def table_sweep(torch, Proto, workload, g, gv, hv, dV, dP, dA, dS, expect, n, steps):
    out = {"unit": "ms per batch of %d proofs, kernel timing off" % n, "points": []}
    for code in (1119, 621, 523):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        t0 = time.perf_counter()
        try:
            p = Proto(g, gv, hv, device=torch.cuda.current_device(), fb_window_bits=code)
        except Exception as e:          # (a box whose memory is partly taken cannot build the widest tables: recorded, not fatal)
            out["points"].append({"fb_window_bits": code, "error": str(e)[:120]})
            continue
        p.synchronize()
        t_ctx = time.perf_counter() - t0
        try:
            dA.zero_()
            for _ in range(2):
                p.verify_batch_device(workload.LABEL, n, dV.data_ptr(), dP.data_ptr(), dA.data_ptr(), dS.data_ptr(), 0, 0)
            p.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                p.verify_batch_device(workload.LABEL, n, dV.data_ptr(), dP.data_ptr(), dA.data_ptr(), dS.data_ptr(), 0, 0)
            p.synchronize()
            ms = (time.perf_counter() - t0) / steps * 1e3
            out["points"].append({"fb_window_bits": code, "windows_per_scalar": p.get_option("fb_windows"), "table_gb": p.get_option("fb_table_bytes") / 1e9,
                                  "context_s": t_ctx, "ms_per_batch": ms, "verifies_per_s": n / ms * 1e3,
                                  "accept_bits_ok": bool((dA.cpu().numpy() == expect).all()), "free_gb_before": free0 / 1e9})
        finally:
            p.close()
    pts = [q for q in out["points"] if "ms_per_batch" in q]
    if len(pts) >= 2:
        out["widest_vs_narrowest"] = {"ms_saved": pts[0]["ms_per_batch"] - pts[-1]["ms_per_batch"], "gb_added": pts[-1]["table_gb"] - pts[0]["table_gb"],
                                      "speedup": pts[0]["ms_per_batch"] / pts[-1]["ms_per_batch"]}
    return out


def load_generators():
    with open(os.path.join(ROOT, "tests", "golden", "u64_golden.json")) as f:
        gens = bytes.fromhex(json.load(f)["generators"])
    return gens, gens[:64], [gens[64 * i:64 * i + 64] for i in range(1, 17)], [gens[64 * i:64 * i + 64] for i in range(17, 49)]


def make_resident_batch(torch, proto, workload, lo, hi, corrupt_every=1024, slice_proofs=1 << 16):
    """Proofs lo..hi of the global synthetic batch, made by the product's batch prover on this GPU in slices and left resident:
    returns (dV [n,64], dP [n,928], expect [n] u8 numpy, seconds spent proving).  One proof in `corrupt_every` (by GLOBAL
    index) gets one bit of l0/l1/n0 flipped and must be rejected."""
    import numpy as np
    n = hi - lo
    dV = torch.empty((n, 64), dtype=torch.uint8, device="cuda")
    dP = torch.empty((n, 928), dtype=torch.uint8, device="cuda")
    dSt = torch.zeros(n, dtype=torch.int32, device="cuda")
    t_prove = 0.0
    for a in range(0, n, slice_proofs):
        b = min(n, a + slice_proofs)
        x = torch.from_numpy(workload.bulk_values(b - a, first=lo + a).view(np.int64)).cuda()
        s = torch.from_numpy(workload.bulk_blindings(b - a, first=lo + a)).cuda()
        r = torch.from_numpy(workload.bulk_prover_randomness(b - a, first=lo + a)).cuda()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        proto.prove_batch_device(workload.LABEL, b - a, x.data_ptr(), s.data_ptr(), r.data_ptr(), dP[a:b].data_ptr(), dV[a:b].data_ptr(),
                                 dSt[a:b].data_ptr())
        proto.synchronize()
        t_prove += time.perf_counter() - t0
        del x, s, r
    if bool(dSt.any().item()):
        print("bench.py: prover reported a status flag", file=sys.stderr)
        sys.exit(4)
    expect = np.ones(n, dtype=np.uint8)
    first_bad = (-lo) % corrupt_every
    idx = np.arange(first_bad, n, corrupt_every, dtype=np.int64)
    if len(idx):
        offs = np.array([workload.corrupt_offset(lo + int(j)) for j in idx], dtype=np.int64)
        ti, to = torch.from_numpy(idx).cuda(), torch.from_numpy(offs).cuda()
        dP[ti, to] = dP[ti, to] ^ 1
        expect[idx] = 0
    torch.cuda.synchronize()
    return dV, dP, expect, t_prove


def dump_outputs(out_dir, rank, arrays):
    """--dump-outputs: each array as out_dir/<name>.npy (float32 / float64; rank r > 0 of a multi-GPU run adds _rank<r> to the name)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(out_dir, name + (f"_rank{rank}" if rank else "") + ".npy"), np.ascontiguousarray(a))


def host_summary():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import hostinfo
    return hostinfo.summary()


def concurrent_callers(proto, label, V, P, expect, thread_counts=(64, 1024)):
    """The reference's calling pattern -- ONE proof per call, T native host threads (tools/cc_callers.c) -- through the library's
    coalescing front end (bppp_u64_verify_one): aggregate rate and per-call latency.  Each point runs ~0.5 s."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import concurrent_callers as cc
    import hostinfo
    from bp_pp_amd import _capi
    import numpy as np
    H = cc.build_harness()
    L = _capi.lib()
    V, P, expect = np.ascontiguousarray(V), np.ascontiguousarray(P), np.ascontiguousarray(np.asarray(expect, dtype=np.uint8))
    out = {"unit": "verifies/s", "entry_point": "bppp_u64_verify_one", "pool_proofs": int(V.shape[0]),
           "note": "T threads each calling verify for ONE proof in a loop (u64_proof.rs:42 from many threads); default coalesce_* options; "
                   "round 3, same pattern through one-proof batched calls: 601 verifies/s at 64 threads"}
    for T in thread_counts:
        cc.run_callers(H, L.bppp_u64_verify_one, [proto._ctx.value], label, V, P, expect, T, 3)
        runs = []
        for _ in range(2):          # the box's host CPUs are shared and capped (cgroup quota): two runs of ~0.5 s, both reported
            thr0, st0 = hostinfo.throttle_stats(), proto.coalesce_stats()
            r = cc.run_callers(H, L.bppp_u64_verify_one, [proto._ctx.value], label, V, P, expect, T, max(20, min(400, 120000 // T)))
            thr1, st1 = hostinfo.throttle_stats(), proto.coalesce_stats()
            r["mean_batch"] = round((st1["requests"] - st0["requests"]) / max(1, st1["batches"] - st0["batches"]), 1)
            r["cgroup_throttled_periods"] = thr1["nr_throttled"] - thr0["nr_throttled"]
            runs.append(r)
        best = max(runs, key=lambda r: r["verifies_per_s"])
        other = runs[1] if best is runs[0] else runs[0]
        best["other_run"] = {"verifies_per_s": other["verifies_per_s"], "p99_ms": other["latency_ms"]["p99"], "max_ms": other["latency_ms"]["max"],
                             "cgroup_throttled_periods": other["cgroup_throttled_periods"]}
        out[f"threads_{T}"] = best
    return out


def cpu_baseline_verify(gens, label, V, P, acc_gpu, sample_note):
    """The oracle, as the timed CPU baseline ONLY: reference-shaped C restatement on the host cores, bounded sample."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import bppp_oracle_c as OC
    m = V.shape[0]
    host = host_summary()
    hw = host["usable_cpus"]           # min(affinity, cgroup CPU quota): what a thread pool here can really keep busy
    t0 = time.perf_counter()
    OC.u64_verify_batch(gens, label, V[:64].copy(), P[:64].copy(), nthreads=1)
    single = 64 / (time.perf_counter() - t0)
    best = None
    ladder = sorted({hw, 2 * hw, max(1, hw // 2)}, reverse=True)
    for th in ladder:
        t0 = time.perf_counter()
        oacc, _ = OC.u64_verify_batch(gens, label, V.copy(), P.copy(), nthreads=th)
        dt = time.perf_counter() - t0
        if best is None or m / dt > best[0]:
            best = (m / dt, th, dt, bool((oacc == acc_gpu[:m]).all()))
    return {"value": best[0], "unit": "verifies/s", "cores": best[1], "kind": "port",
            "sample": f"{sample_note}, reference-shaped C restatement (oracle/bppp_ref.c); best of thread counts {ladder} = "
                      f"{best[1]} threads, {best[2]:.2f} s wall; {host['cpu_model']}: {host['affinity_cpus']} CPUs in the affinity mask, "
                      f"cgroup CPU quota {host['cgroup_cpu_quota']}",
            "host": host, "single_thread_value": single, "agrees_with_gpu": best[3]}


def run_verify(args):
    import numpy as np
    import torch
    import torch.distributed as dist
    world, rank, local_rank = setup_dist(args)
    from bp_pp_amd import U64RangeProofProtocol, synth as workload
    from bp_pp_amd.distributed import all_reduce_reject_count, shard_range

    gens, g, gv, hv = load_generators()
    total = args.total_proofs
    lo, hi = shard_range(total, rank, world)
    n = hi - lo
    t0 = time.time()
    proto = U64RangeProofProtocol(g, gv, hv, device=local_rank, fb_window_bits=args.fb_window_bits)
    proto.synchronize()
    t_ctx = time.time() - t0
    t0 = time.time()
    dV, dP, expect, t_prove = make_resident_batch(torch, proto, workload, lo, hi)
    t_setup = time.time() - t0

    dA = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dS = torch.zeros(n, dtype=torch.int32, device="cuda")
    dR = torch.zeros(1, dtype=torch.int32, device="cuda")
    # one explicit stream for the verify kernels AND the accept-reduce, so that NCCL's stream dependency covers the kernels that
    # write the reject count (the context's own streams are non-blocking: not ordered against torch's default stream)
    stream = torch.cuda.Stream()
    proto.set_stream(stream.cuda_stream)

    def step(nn=n, acc=dA, rej=dR):
        with torch.cuda.stream(stream):
            proto.verify_batch_device(workload.LABEL, nn, dV.data_ptr(), dP.data_ptr(), acc.data_ptr(), dS.data_ptr(), 0, rej.data_ptr())
            if nn == n:
                all_reduce_reject_count(rej)            # the single accept-reduce (4 bytes over RCCL/xGMI); no-op at N=1

    dist_on = dist.is_initialized()

    def fence():
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    # Pass 1 -- what `value` is: EXACTLY args.steps steps on the plan a caller gets (kernel timing off: the helper stream carries the
    # fixed-base half of C0, nothing wraps the launches in events).
    t_start = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t_start
    plan_shipping = proto.last_plan()

    # correctness of what was just timed (untimed): accept bits == expectation, global reject count == corrupted proofs
    acc = dA.cpu().numpy()
    st = dS.cpu().numpy()
    ok_local = bool((acc == expect).all() and not st.any())
    rejects = int(dR.item())
    expected_rejects = len(range(0, total, 1024))
    if args.dump_outputs:
        # what a caller of verify_batch_device receives from the last timed step: accept bit and status word per proof of this rank's
        # shard, and the all-reduced reject count
        dump_outputs(args.dump_outputs, rank, {"accept": acc.astype(np.float32), "status": st.astype(np.float64),
                                               "reject_count": np.array([rejects], dtype=np.float64)})

    kernel_times, elapsed_timed, plan_timed = {}, None, None
    if args.full:
        # Pass 2 -- diagnostics only: the same steps with per-kernel HIP events on the launch stream (the C0 halves then run back to back so
        # that the kernel times add up; below 2^17 proofs the plan also loses its side-by-side kernels).  kernels_ms_per_step, roofline
        # and roofline_valu come from here; its wall time is reported beside pass 1's and must agree with it when the plans are the same.
        proto.enable_timing(True)
        proto.timings(reset=True)
        fence()
        t_start = time.perf_counter()
        for _ in range(args.steps):
            step()
        fence()
        elapsed_timed = time.perf_counter() - t_start
        kernel_times = proto.timings(reset=True)
        plan_timed = proto.last_plan()
        proto.enable_timing(False)
        ok_local = ok_local and bool((dA.cpu().numpy() == expect).all() and not dS.any().item()) and int(dR.item()) == rejects
    global SHARED_INV
    SHARED_INV = shared_inv_of(plan_shipping)

    def max_over_ranks(x):
        t = torch.tensor([x], dtype=torch.float64, device="cuda")
        if dist_on:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def timed_share(m, what):
        """the first m proofs of the resident batch as a call of their own, kernel timing off (the plan a caller gets)"""
        dAm = torch.zeros(m, dtype=torch.uint8, device="cuda")
        dRm = torch.zeros(1, dtype=torch.int32, device="cuda")
        reps = max(args.steps, 10)
        step(m, dAm, dRm)
        fence()
        best = None
        for _ in range(2):                   # two rounds of `reps` calls, the faster one reported (both listed)
            t = time.perf_counter()
            for _ in range(reps):
                step(m, dAm, dRm)
            fence()
            t = (time.perf_counter() - t) / reps
            best = (t, [t * 1e3]) if best is None else (min(t, best[0]), best[1] + [t * 1e3])
        return {"workload": what, "value": m / best[0], "unit": "verifies/s", "ms_per_step": best[0] * 1e3, "rounds_ms": [round(x, 3) for x in best[1]],
                "calls_per_round": reps, "plan": proto.last_plan(), "accept_bits_ok": bool((dAm.cpu().numpy() == expect[:m]).all())}

    # BENCH_LITE=1 (diagnostic): the headline passes, configs[1] and the shares only
    lite = bool(os.environ.get("BENCH_LITE"))
    secondary = args.full and not args.no_secondary
    # ---- secondary measurements, reported separately and never as `value`
    cfg1 = rlc = host_path = None
    if world == 1 and secondary:
        m = min(n, 1 << 16)
        cfg1 = timed_share(m, f"BASELINE configs[1]: the first {m} proofs of the same resident batch on one GPU")
    if world == 1 and secondary and not lite:
        m = min(n, 1 << 16)
        V16, P16 = dV[:m].cpu().numpy(), dP[:m].cpu().numpy()
        proto.verify_batch(V16, P16, workload.LABEL)
        t_h = None
        for _ in range(3):           # best of three: the calling thread does the pageable staging, and the boxes' cgroups throttle it at times
            t0 = time.perf_counter()
            hacc, _ = proto.verify_batch(V16, P16, workload.LABEL)
            t0 = time.perf_counter() - t0
            t_h = t0 if t_h is None else min(t_h, t0)
        host_path = {"value": m / t_h, "unit": "verifies/s", "ms_per_batch": t_h * 1e3, "proofs": m,
                     "accept_bits_ok": bool((hacc == expect[:m]).all()),
                     "note": "bppp_u64_verify_batch with pageable host buffers: 65 MB host-to-device per batch included"}
        # the same proofs in the reference's wire form (33-byte SEC1 points: 525 + 33 bytes per proof instead of 928 + 64 over PCIe,
        # and 14 square roots per proof on the device to decompress them)
        from bp_pp_amd import wire
        C33 = np.frombuffer(b"".join(wire.compress_point(bytes(V16[i])) for i in range(m)), dtype=np.uint8).reshape(m, 33).copy() if m <= (1 << 16) else None
        if C33 is not None:
            P525 = np.frombuffer(b"".join(wire.abi_to_sec1(bytes(P16[i])) for i in range(m)), dtype=np.uint8).reshape(m, 525).copy()
            proto.verify_batch_sec1(C33, P525, workload.LABEL)
            t_s = None
            for _ in range(3):
                t0 = time.perf_counter()
                sacc, _ = proto.verify_batch_sec1(C33, P525, workload.LABEL)
                t0 = time.perf_counter() - t0
                t_s = t0 if t_s is None else min(t_s, t0)
            host_path["sec1_form"] = {"value": m / t_s, "unit": "verifies/s", "ms_per_batch": t_s * 1e3, "accept_bits_ok": bool((sacc == expect[:m]).all()),
                                      "note": "bppp_u64_verify_batch_sec1: 36.6 MB over PCIe instead of 65 MB, then on-device decompression"}
        if n > m:
            # the whole batch from pageable host memory (1 GB at 2^20): in parts that grow -- the first 2^17 proofs, then what can be
            # uploaded while that part is verified, 7 times as much (bppp_u64.hip: verify_host_impl) -- and, for comparison, uploaded in
            # one piece before the first kernel
            Vh, Ph = dV.cpu().numpy(), dP.cpu().numpy()
            full = {}
            for name, chunk in (("pipelined", 1 << 17), ("upload_first", 0)):
                proto.set_option("host_chunk", chunk)
                proto.verify_batch(Vh, Ph, workload.LABEL)          # untimed: grows the context's staging buffers to this size
                t_h = None
                for _ in range(2):
                    t0 = time.perf_counter()
                    hacc, _ = proto.verify_batch(Vh, Ph, workload.LABEL)
                    t0 = time.perf_counter() - t0
                    t_h = t0 if t_h is None else min(t_h, t0)
                full[name] = {"value": n / t_h, "ms_per_batch": t_h * 1e3, "accept_bits_ok": bool((hacc == expect).all())}
            proto.set_option("host_chunk", 1 << 17)
            host_path["full_batch"] = dict(full, proofs=n, unit="verifies/s")
            del Vh, Ph
    # one GPU's share of the same batch when it is split over 8 / 4 / 2 GPUs (shard_range: contiguous, so the first 2^20 / N proofs ARE
    # rank 0's share), on the shipping plan: the only measurable determinant of the N-GPU number on a one-GPU box
    shares = {}
    if world == 1 and secondary:
        for lg in (17, 18, 19):
            if n >= (1 << lg):
                shares[lg] = timed_share(1 << lg, f"one GPU's share of BASELINE configs[2]'s {total >> lg}-GPU split: the first {1 << lg} proofs of the same resident batch")
    shard17 = shares.get(17)
    # the reference's WIRE form resident on the device (reciprocal.rs:37-59: 33-byte SEC1 points -- 525 B per proof + 33 B per commitment):
    # the same proofs, written in that form by the product's prover, decompressed on the device (14 square roots per proof) and verified
    sec1_dev = None
    if world == 1 and secondary and not lite:
        sec1_dev = measure_sec1_device(torch, proto, workload, n, expect, max(3, min(args.steps, 5)), stream)
    callers = None
    if world == 1 and secondary and not under_profiler() and not lite:
        m = min(n, 4096)
        callers = concurrent_callers(proto, workload.LABEL, dV[:m].cpu().numpy(), dP[:m].cpu().numpy(), expect[:m])
    call_latency = None
    if world == 1 and secondary and not lite:
        # one call of a few proofs, host buffers in and out (the reference's own usage is one verify / prove at a time: BASELINE
        # configs[0], benches/range_proof.rs): what a caller waits for, not a throughput
        call_latency = {"unit": "ms per call, host buffers", "note": "bppp_u64_verify_batch / bppp_u64_prove_batch on n proofs, median of 7 calls; "
                        "the reference's bench on an M3 Pro core: 3.808 ms per verify, 14.361 ms per prove (BASELINE.md)"}
        xs, ss, rs = workload.bulk_values(1024), workload.bulk_blindings(1024), workload.bulk_prover_randomness(1024)
        for m in (1, 64, 1024):
            Vm, Pm = dV[:m].cpu().numpy(), dP[:m].cpu().numpy()
            tv, tp, okm = [], [], True
            for it in range(8):
                t0 = time.perf_counter()
                a_m, _ = proto.verify_batch(Vm, Pm, workload.LABEL)
                tv.append(time.perf_counter() - t0)
                okm &= bool((a_m == expect[:m]).all())
                t0 = time.perf_counter()
                pp, cc, st_m = proto.prove_batch(xs[:m], ss[:m], rs[:m], workload.LABEL)
                tp.append(time.perf_counter() - t0)
                okm &= not bool(st_m.any())
            a_m, _ = proto.verify_batch(cc, pp, workload.LABEL)          # what the small prove calls made verifies
            okm &= bool(a_m.all())
            call_latency[f"n{m}"] = {"verify_ms": float(np.median(tv[1:]) * 1e3), "prove_ms": float(np.median(tp[1:]) * 1e3), "ok": okm}
    if secondary and not lite:
        dA2 = torch.zeros(n, dtype=torch.uint8, device="cuda")
        dR2 = torch.zeros(1, dtype=torch.int32, device="cuda")
        seed = os.urandom(32)

        def rlc_step():
            with torch.cuda.stream(stream):
                proto.verify_batch_rlc_device(workload.LABEL, n, dV.data_ptr(), dP.data_ptr(), dA2.data_ptr(), seed, dS.data_ptr(), dR2.data_ptr())
                all_reduce_reject_count(dR2)

        def rlc_measure():
            """-> (seconds for args.steps steps, per-kernel ms per step of one more step with kernel timing on, the group sizes used)"""
            proto.set_option("rlc_history", 0)
            rlc_step()                      # first call on this input stream: no history yet (round 4's group sizes) ...
            fence()
            rlc_step()                      # ... the following ones plan with the previous call's reject rate (plan_core.h: plan_rlc)
            fence()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                rlc_step()
            fence()
            t = max_over_ranks(time.perf_counter() - t0)
            proto.enable_timing(True)
            proto.timings(reset=True)
            rlc_step()
            fence()
            kt = proto.timings(reset=True)
            proto.enable_timing(False)
            used = {"superchunk": proto.get_option("last_rlc_superchunk"), "chunk": proto.get_option("last_rlc_chunk"),
                    "reject_ppm_planned_with": proto.get_option("rlc_reject_ppm") if proto.get_option("rlc_has_history") else None}
            return t, {k: v["total_ms"] for k, v in kt.items() if v["launches"]}, used

        t_r, kt_r, used_r = rlc_measure()
        rlc = {"value": total * args.steps / t_r, "unit": "verifies/s", "ms_per_step": t_r / args.steps * 1e3,
               "accept_bits_equal_exact_mode": bool((dA2 == dA).all().item()) and int(dR2.item()) == rejects,
               "kernels_ms_per_step": kt_r, "group_sizes": used_r,
               "roofline_valu": valu_roofline("k_verify_round", kt_r.get("k_verify_round", 0.0) / 4, n, 1) if kt_r.get("k_verify_round") else None,
               "note": "optional mode (bppp_u64_verify_batch_rlc_device) on the SAME batch (1/1024 proofs corrupted): random linear combinations "
                       "of the final checks, failing groups re-checked exactly; group sizes follow the previous call's reject rate (here: no "
                       "bucket stage -- every superchunk would hold a bad proof -- and chunks of 32); NOT the headline metric"}
        # the regime the bucket stage is for: every proof valid.  The corrupted bytes are flipped back for this measurement only.
        bad_idx = np.nonzero(expect == 0)[0]
        if expected_rejects:        # a GLOBAL condition: every rank takes part in the collectives below, with or without local repairs
            ti = torch.from_numpy(bad_idx).cuda()
            to = torch.from_numpy(np.array([workload.corrupt_offset(lo + int(j)) for j in bad_idx], dtype=np.int64)).cuda()
            if len(bad_idx):
                dP[ti, to] = dP[ti, to] ^ 1
            torch.cuda.synchronize()
            t_v, kt_v, used_v = rlc_measure()
            rlc["all_valid"] = {"value": total * args.steps / t_v, "unit": "verifies/s", "ms_per_step": t_v / args.steps * 1e3,
                                "all_accepted": bool(dA2.all().item()) and int(dR2.item()) == 0,
                                "kernels_ms_per_step": kt_v, "group_sizes": used_v,
                                "note": "same batch with the corrupted bytes restored: the bucket (Pippenger) stage passes every superchunk"}
            if len(bad_idx):
                dP[ti, to] = dP[ti, to] ^ 1
            torch.cuda.synchronize()

    # BASELINE configs[3] and configs[4] at one GPU's size, so that the driver's default run records them too (their full lines:
    # --workload prove, --workload recip256).  Same measurement code as those workloads, reduced cpu_baseline samples.
    prove14 = recip15 = None
    ok_extra = True
    if world == 1 and secondary and not lite:
        import bench_other
        keep = ("metric", "value", "unit", "ms_per_step", "timing_pass_ms_per_step", "steps", "config", "roofline", "kernels_ms_per_step", "cpu_baseline", "ct_prover")
        r, okp = bench_other.measure_prove(args, proto, gens, 1 << 14, cpu_baseline=not args.no_cpu_baseline, cpu_sample=2048)
        prove14 = {k: r[k] for k in keep if k in r}
        prove14["proofs_verify"] = okp
        ok_extra = okp

    # every rank's own clock over the timed region, gathered (what the max below is taken over)
    per_rank_ms = [elapsed / args.steps * 1e3]
    if dist_on:
        mine = torch.tensor([elapsed / args.steps * 1e3], dtype=torch.float64, device="cuda")
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank_ms = [float(x.item()) for x in allr]
    ranks = {"backend": (dist.get_backend() if dist_on else None), "rccl_nranks": (world if dist_on and dist.get_backend() == "nccl" else 0),
             "per_rank_ms": [round(x, 3) for x in per_rank_ms], "max_ms": round(max(per_rank_ms), 3), "one_device_dry_run": bool(os.environ.get("BENCH_ONE_DEVICE"))}
    elapsed = max_over_ranks(elapsed)
    ok_all = torch.tensor([1 if ok_local else 0], dtype=torch.int32, device="cuda")
    if dist_on:
        dist.all_reduce(ok_all, op=dist.ReduceOp.MIN)
    ok = bool(ok_all.item()) and rejects == expected_rejects

    ok_timing = True
    timing_pass = None
    if args.full:
        # the two passes must tell the same story when they ran the same plan: more than 2 % apart fails the run
        elapsed_timed = max_over_ranks(elapsed_timed)
        ms_ship, ms_timed = elapsed / args.steps * 1e3, elapsed_timed / args.steps * 1e3
        same_plan = plan_shipping == plan_timed
        timing_pass = {"ms_per_step": ms_timed, "plan": plan_timed, "same_plan_as_value": same_plan, "ratio_to_value_pass": ms_timed / ms_ship,
                       # (checked where it means something: the same plan, steps of 50 ms or more -- the ~25 event pairs of a timed step are noise
                       # there --, and every rank on a GPU of its own: the one-device dry run's ranks take turns on one chip)
                       "agrees_within_2pct": (abs(ms_timed / ms_ship - 1.0) <= 0.02) if (same_plan and ms_ship >= 50.0 and not os.environ.get("BENCH_ONE_DEVICE")) else None,
                       "note": "second pass of the same steps with per-kernel HIP events (C0's halves back to back): the source of kernels_ms_per_step, "
                               "roofline and roofline_valu, never of `value`; a plan that differs (below 2^17 proofs per GPU the timed pass has no "
                               "side-by-side kernels, at 2^17 .. 2^18 no twin chains) or a step under 50 ms (the events themselves show), or ranks sharing one device, is not "
                               "comparable and not checked"}
        ok_timing = timing_pass["agrees_within_2pct"] is not False
    if rank == 0:
        value = total * args.steps / elapsed
        diagnostics = secondaries = {}
        if args.full:
            dom_name, dom_t = max(kernel_times.items(), key=lambda kv: kv[1]["total_ms"])
            avg_ms = dom_t["total_ms"] / max(1, dom_t["launches"])
            achieved = ALGO_BYTES_PER_VERIFY * n / (avg_ms * 1e-3) / 1e9
            traffic_step = pmc_traffic_per_step(kernel_times, args.steps, n)
            diagnostics = {
                "roofline": {
                    "bound": "hbm",
                    "kernel": dom_name,
                    "achieved": achieved,
                    "peak": HBM_PEAK_GBS,
                    "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS,
                    "traffic": pmc_traffic(dom_name, n),
                    "avg_launch_ms": avg_ms,
                    "launches_per_step": dom_t["launches"] / args.steps,
                    "algorithmic_bytes_per_launch": ALGO_BYTES_PER_VERIFY * n,
                    "traffic_all_kernels_per_step": traffic_step,
                    "traffic_all_kernels_over_algorithmic": (traffic_step / (ALGO_BYTES_PER_VERIFY * n)) if traffic_step else None,
                    "note": "256-bit modular integer path: VALU issue bound, HBM fraction is small by construction "
                            "(SURVEY.md 8d); roofline_valu is the ceiling that binds.  traffic* come from the committed rocprofv3 --pmc "
                            "summaries and are null unless those were collected on the device code this run loaded (pmc_matches_build)",
                },
                "pmc_matches_build": pmc_matches_build(),
                "roofline_valu": valu_roofline(dom_name, avg_ms, n, 8 if dom_name in FB_KERNELS else 1),
                "kernels_ms_per_step": {k: v["total_ms"] / args.steps for k, v in kernel_times.items() if v["launches"]},
                "timing_pass": timing_pass,
            }
            secondaries = {
                "configs1_2pow16": cfg1,
                "shard_2pow17": shard17,
                "shard_2pow18": shares.get(18),
                "shard_2pow19": shares.get(19),
                "predicted_scaling": predicted_scaling(total, elapsed / args.steps * 1e3, shares) if world == 1 else None,
                "concurrent_callers": callers,
                "rlc_mode": rlc,
                "host_buffer_path": host_path,
                "sec1_device": sec1_dev,
                "call_latency": call_latency,
                "prove_2pow14": prove14,
                "recip256_2pow15": recip15,
            }
        result = {
            "metric": "u64 range-proof batch verifies/sec",
            "value": value,
            "unit": "verifies/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "u32",
            "data": "synthetic",
            "config": {
                "workload": f"batch verify ONE fixed batch of {total} independent u64 range proofs (BASELINE configs[2]; "
                            f"{'all resident on one GPU' if world == 1 else f'sharded contiguously over {world} GPUs, {n} proofs per GPU'}), "
                            "exact per-proof mode, shared generators, inputs resident in HBM, 1/1024 proofs corrupted, one 4-byte "
                            "reject-count all-reduce per step",
                "total_proofs_per_step": total,
                "proofs_per_gpu": n,
                "fb_window_bits": proto.get_option("fb_window_bits"),            # a window code: 523 = 5 windows of 24 bits + 6 of 23 per scalar (include/bppp.h)
                "fb_window_bits_hi": proto.get_option("fb_window_bits_hi"),      # > 0: the first fb_hi_bases generators (g, g_vec) in a second, wider table
                "fb_hi_bases": proto.get_option("fb_hi_bases"),
                "fb_window_bits_chosen_by": "--fb-window-bits" if args.fb_window_bits else "the library, from the HBM free at context creation",
                "label": workload.LABEL.decode(),
                "parallelism": f"shard{world}" if world > 1 else "single",
                "plan": plan_shipping,               # the launch plan of the timed steps (include/bppp.h: "last_verify_plan")
                "kernel_timing_during_value": False,
                "full": args.full,                   # --full: the diagnostics and secondary objects below were measured too
            },
            **diagnostics,
            "accept_bits_ok": ok,
            "reject_count_all_reduced": rejects,
            "ranks": ranks,
            **secondaries,
            "setup_s": {"context_tables": t_ctx, "inputs_and_gpu_batch_prove": t_setup, "gpu_batch_prove_only": t_prove},
            "prover": {"proofs_per_s_device_buffers": n / t_prove, "note": "setup only; see --workload prove for BASELINE configs[3]"},
            "device_bytes": proto.device_bytes(),
        }
        if world == 1 and args.full and not args.no_cpu_baseline:
            m = min(args.cpu_sample, n)
            result["cpu_baseline"] = cpu_baseline_verify(gens, workload.LABEL, dV[:m].cpu().numpy(), dP[:m].cpu().numpy(), acc,
                                                         f"first {m} proofs of the same batch")
    proto.close()
    if rank == 0:
        if world == 1 and secondary and not lite and n >= (1 << 17):
            # what the fixed-base tables buy: the same resident batch through contexts of 13, 12 and 11 windows per scalar (window codes
            # 1119 / 621 / 523, include/bppp.h) created one after the other on this box -- table bytes, what the context costs to create,
            # ms per batch.  The library takes 11 windows (210 GB) on an empty MI355X unless the caller gives it a table budget
            # (bppp_wnla_ctx_create_budget); this is the price list that decision is made from.  Secondary, never `value`.
            result["table_sweep"] = table_sweep(torch, U64RangeProofProtocol, workload, g, gv, hv, dV, dP, dA, dS, expect, n, max(3, min(args.steps, 5)))
        if world == 1 and secondary and not lite:
            # configs[4]'s shape needs tables of its own (769 generators: 97 GB at the 18 bits the library picks on a free device): measured
            # after the u64 context -- 152 GB of tables since round 5 -- has been released, so that the width it gets is the one a caller
            # who only runs this protocol gets
            del dV, dP
            torch.cuda.empty_cache()
            import bench_other
            keep = ("metric", "value", "unit", "ms_per_step", "timing_pass_ms_per_step", "steps", "config", "roofline", "kernels_ms_per_step", "cpu_baseline", "ct_prover")
            r, okr = bench_other.measure_recip256(args, 1 << 15, 0, cpu_baseline=not args.no_cpu_baseline, rlc=True)
            result["recip256_2pow15"] = {k: r[k] for k in keep + ("rlc_mode", "accept_bits_ok", "device_bytes") if k in r}
            ok_extra = ok_extra and okr
            # the crate's generic `wnla` and `circuit` API at 2^16 instances (their own lines: --workload wnla / circuit)
            saved_w = args.fb_window_bits
            args.fb_window_bits = args.fb_window_bits or 16
            try:
                rw, okw = bench_other.measure_wnla(args, 1 << 16, cpu_baseline=not args.no_cpu_baseline, cpu_sample=128)
                rc_, okc = bench_other.measure_circuit(args, 1 << 16, name="mixed_k2", cpu_baseline=not args.no_cpu_baseline, cpu_sample=64)
            finally:
                args.fb_window_bits = saved_w
            gkeep = keep + ("roofline_valu", "accept_bits_ok")
            result["wnla_16_32_2pow16"] = {k: rw[k] for k in gkeep if k in rw}
            result["circuit_mixed_k2_2pow16"] = {k: rc_[k] for k in gkeep if k in rc_}
            for key, wl in (("wnla_16_32_2pow16", "wnla"), ("circuit_mixed_k2_2pow16", "circuit")):
                result[key]["note"] = (f"reduced copy of `python bench.py --workload {wl}` on 16-bit fixed-base tables (17 windows per scalar, built in a fraction of a "
                                       "second, so that the default run stays short; config.fb_window_bits says so); the workload's own line runs on the layout the "
                                       "library picks on a free device (11 windows) and is about a tenth faster (profiles/r06/r06_zz_cmd_*.txt)")
            ok_extra = ok_extra and okw and okc
        print(json.dumps(result), flush=True)
    if dist_on:
        dist.destroy_process_group()
    if not ok_timing and rank == 0:
        print(f"bench.py: the kernel-timing pass ({ms_timed:.3f} ms) and the value pass ({ms_ship:.3f} ms) ran the same plan and differ by more than 2 %", file=sys.stderr)
    if not (ok and ok_extra and ok_timing):
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", choices=["verify", "prove", "recip256", "wnla", "circuit"], default="verify")
    ap.add_argument("--statement", default="mixed_k2", help="--workload circuit: a statement of tests/golden/statements_generic.json (mixed_k2, ac_works, fm_nv1)")
    ap.add_argument("--total-proofs", type=int, default=0, help="size of the fixed global batch (default: 2^20 verify, 2^14 prove, 2^18 recip256, 2^16 wnla / circuit)")
    ap.add_argument("--fb-window-bits", type=int, default=0)
    ap.add_argument("--cpu-sample", type=int, default=8192, help="proofs verified by the CPU baseline (rank 0, N=1): ~10-20 s of host work")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the secondary measurements (configs[1], RLC mode, host-buffer path)")
    ap.add_argument("--no-session-rates", action="store_true", help="do not run tools/ratebench (the profiler command lines pass this)")
    ap.add_argument("--full", action="store_true",
                    help="default workload: also the kernel-timing pass, rooflines, session issue rates, the secondary objects and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="default workload: write what the last timed step computed as DIR/<name>.npy")
    args = ap.parse_args()
    if args.dump_outputs and args.workload != "verify":
        ap.error("--dump-outputs is implemented for the default workload (--workload verify) only")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        sys.exit(launch_ranks(args.gpus))
    # the chip's issue rates and clock, measured by a child process NOW: nothing in this process has touched the GPU yet (torch is
    # not even imported), and the GPU is idle.  Only roofline_valu uses them: the default workload measures them under --full alone.
    if int(os.environ.get("RANK", "0")) == 0 and not args.no_session_rates and not under_profiler() and (args.full or args.workload != "verify"):
        session_rates(measure=True)
    if args.workload == "verify":
        args.total_proofs = args.total_proofs or (1 << 20)
        run_verify(args)
    elif args.workload in ("wnla", "circuit"):
        import bench_other
        args.total_proofs = args.total_proofs or (1 << 16)
        bench_other.run_generic(args)
    else:
        import bench_other
        args.total_proofs = args.total_proofs or ((1 << 14) if args.workload == "prove" else (1 << 18))
        (bench_other.run_prove if args.workload == "prove" else bench_other.run_recip256)(args)


if __name__ == "__main__":
    main()
