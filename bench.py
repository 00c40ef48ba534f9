#!/usr/bin/env python
"""bench.py — BASELINE.json metric on MI355X:
  "G1 MSM scalars/sec at 2^24 + sumcheck-prover ms at 2^20 vars (1/8 GPU)".

One step = one KZG commitment (Pippenger G1 MSM) over 2^24 BN254 scalars per
GPU, inputs (SRS bases + scalars) already resident in HBM.  With N GPUs the
commitment is to a degree N*2^24 polynomial: rank r owns bases/scalars
[r*2^24, (r+1)*2^24) and the per-rank partial sums are combined by one RCCL
allgather (weak scaling; value = N*2^24 / max-over-ranks time).

A plain run does only that: it sets up, warms up, times the steps, writes the
last step's commitment if --dump-outputs is given, and prints the result line.
Everything below runs only with --full.

With --full, the sumcheck prover (SumcheckProof::prove, h = g1*g2*g3, degree 3)
at 2^20 variables is reported in `sumcheck` with its own HBM roofline (with N
ranks the 2^20 tables are sharded by the high index bits: strong scaling), and
configs C4 (ML-PCS commit + open, 2^22), the Logup column and C5 (HyperPlonk
prove, 2^20-row traces) get their own entries.  The CPU baseline is the oracle's C
restatement of the reference algorithm (single thread, like the reference,
which has no rayon), timed on a bounded sample on rank 0.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
       (N > 1 via torch.distributed.run, one process per GPU)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "quill-zkvm_amd"))

HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
# hardware issue bound of the 29-bit Fq multiply: v_mad_u64_u32 lane-ops/s
# measured on MI355X (profiles/r01_isa_rates.json, every CU issuing) / the 162
# partial products of one 9 x 9-limb Montgomery product (81 a*b + 81 m*p)
VMAD_LANE_OPS_PER_S = 3.1186e13
MADS_PER_FQ_MUL = 162
# random whole-row (128 B, one coalesced request per row) gathers per second over a
# 16 GiB table, micro/gather_bench.hip "coop 8 lanes x 16B of 128B" (profiles/r05_gather_bench.txt)
COOP_GATHER_ROWS_PER_S = 3.37e10
LOGUP_BYTES_PER_ROW = 128  # 3 x 32 B table reads + 32 B column write
MSM_BYTES_PER_SCALAR = 96  # 32 B scalar + 64 B affine base
MSM_FQMUL_PER_SCALAR = 176  # 16 signed windows x 11 Fq mults


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, run every other leg and check: the commitment "
                         "check, the Fq-mul microbenchmark, the PMC traffic passes, sumcheck, "
                         "zero-check, the other MSM legs, ML-PCS open, Logup, HyperPlonk and "
                         "the CPU baselines (each still has its own switch below)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float64)")
    ap.add_argument("--log-msm", type=int, default=24)
    ap.add_argument("--log-msm-small", type=int, default=20,
                    help="config 2: a resident 2^k MSM with its own SRS (window size chosen "
                         "for 2^k), commitment checked (0: skip)")
    ap.add_argument("--log-sumcheck", type=int, default=20)
    ap.add_argument("--no-sumcheck", action="store_true")
    ap.add_argument("--log-mle", type=int, default=22,
                    help="config C4: ML-PCS commit + open at 2^k evaluations (0: skip)")
    ap.add_argument("--log-logup", type=int, default=22,
                    help="Logup column rows per GPU (log2); 0 disables")
    ap.add_argument("--log-hp-rows", type=int, default=20,
                    help="config C5: HyperPlonk prove, fibonacci + modified fibonacci traces "
                         "at 2^k rows (0: skip)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-hp-rows-log", type=int, default=12,
                    help="rows (log2) of the C5 CPU-baseline sample (HyperPlonk prove in C)")
    ap.add_argument("--cpu-sample-log", type=int, default=20,
                    help="log2 size of the CPU-baseline MSM sample (a prefix of the workload)")
    ap.add_argument("--no-oneshot", dest="oneshot", action="store_false",
                    help="skip the one-shot-bases leg: the headline MSM over the same bases "
                         "uploaded with qg_bases_upload (one table, no window-shifted copies)")
    ap.add_argument("--no-host-input", dest="host_input", action="store_false",
                    help="skip the drop-in leg: the same commitment from host memory "
                         "(qg_kzg_commit, H2D inside the timed region)")
    ap.add_argument("--no-traffic", action="store_true",
                    help="skip the two rocprofv3 PMC passes that measure HBM traffic")
    ap.add_argument("--no-scaling-modes", action="store_true",
                    help="skip the strong-scaling MSM (fixed 2^log-msm total) and weak-scaling "
                         "sumcheck (2^log-sumcheck per GPU) legs")
    ap.add_argument("--detail-out", default=os.path.join(ROOT, "gpurun_out", "bench_detail.json"),
                    help="file for the full report (per-shape PMC tables, notes); stdout "
                         "carries only the compact line ('' disables)")
    ap.add_argument("--traffic-probe", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args()


SC_KERNELS = ("k_sc_big", "k_sc_round", "k_sc_persist", "k_sc_finish", "k_sc_slice", "k_sc_tail")
# qg_trace_marker tags: an empty kernel of `tag` work-groups at the start of each
# leg lets profiles/kstats.py --legs and pmc_traffic.py attribute every dispatch
# to its leg (kernels of one grid shape recur across legs)
LEG_TAGS = {"msm_2p24": 1, "sumcheck": 2, "msm_host": 3, "scaling": 4, "mle_open": 5, "logup": 6,
            "hyperplonk": 7, "msm_2p20": 8, "cpu_baseline": 9, "probe_msm": 10,
            "probe_sumcheck": 11, "probe_logup": 12, "probe_mle": 13, "probe_cal": 14,
            "msm_oneshot": 15, "zerocheck": 16}


def traffic_probe(args):
    """Child of the PMC passes (pmc_traffic.py): one MSM, then one sumcheck."""
    import quill_amd as q
    from quill_amd.hyperplonk import VirtualPolyExpr as E, sumcheck_prove_device
    dev = q.Device(0)
    n = 1 << args.log_msm
    srs = q.Srs.generate(dev, TAU, n)
    scalars = q.DeviceVec(dev, n).fill_random(0x5155494C4C + 2)
    dev.trace_marker(LEG_TAGS["probe_msm"])
    srs.msm_dev(scalars)
    srs.close()
    scalars.close()
    # FETCH_SIZE calibration launches: known counts of random 128-B row gathers
    # (the accumulate's pattern) and of 16-B-per-lane streaming bytes
    import pmc_traffic
    dev.trace_marker(LEG_TAGS["probe_cal"])
    dev.microbench_fetch(pmc_traffic.CAL_ROWS, pmc_traffic.CAL_GATHERS)
    if not args.no_sumcheck:
        N = 1 << args.log_sumcheck
        tabs = [q.DeviceVec(dev, N).fill_random(0x5155494C4C + 3 + 7 * i) for i in range(3)]
        dev.trace_marker(LEG_TAGS["probe_sumcheck"])
        sumcheck_prove_device(dev, args.log_sumcheck, tabs, E.Input(0) * E.Input(1) * E.Input(2),
                              0, q.Transcript(b"sumcheck_bench"))
        for t in tabs:
            t.close()
    if args.log_logup > 0:
        from quill_amd.logup import logup_column_device
        n = 1 << args.log_logup
        tabs = [q.DeviceVec(dev, n).fill_random(0x5155494C4C + 5 + 11 * i) for i in range(3)]
        out = q.DeviceVec(dev, n)
        dev.trace_marker(LEG_TAGS["probe_logup"])
        logup_column_device(dev, args.log_logup, tabs, E.Input(0) + E.Const(LOGUP_A) * E.Input(1),
                            LOGUP_BETA, out, E.Input(2))
        for t in tabs + [out]:
            t.close()
    if args.log_mle > 0:
        # ML-PCS commit + open (S-polynomial NTT passes, suffix-Horner, MSMs)
        from quill_amd import KZG, Transcript
        n = 1 << args.log_mle
        kzg = KZG(dev, q.Srs.generate(dev, TAU, n), n - 1)
        poly = q.DeviceVec(dev, n).fill_random(0x5155494C4C + 4)
        dev.trace_marker(LEG_TAGS["probe_mle"])
        C = kzg.srs.msm_dev(poly)
        t = Transcript(b"MLPCS bench")
        t.append_g1(C)
        kzg.open_dev(poly, n, [t.draw_field_element() for _ in range(args.log_mle)], t)
        poly.close()
        kzg.srs.close()
    dev.close()


def measure_traffic(args):
    import pmc_traffic
    probe = ["--log-msm", str(args.log_msm), "--log-sumcheck", str(args.log_sumcheck),
             "--log-logup", str(args.log_logup), "--log-mle", str(args.log_mle)]
    if args.no_sumcheck:
        probe.append("--no-sumcheck")
    try:
        return pmc_traffic.collect(probe)
    except Exception as e:  # reported, never substituted
        return {"error": str(e)[-600:]}


TAU = 0x5155494C4C2D53525321  # fixed synthetic trapdoor


_T0 = time.perf_counter()


def _progress(rank, msg):
    """one stderr line per bench leg (rank 0): keeps long runs visibly alive;
    stdout carries only the JSON line"""
    if rank == 0:
        print(f"[bench {time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def launch_plan(gpus, env):
    """What `--gpus N` means for this process: "run" (this process is one rank,
    or the only one), "launch" (no outer launcher and N > 1: start N rank
    processes as children), or an error string (an outer launcher whose
    WORLD_SIZE disagrees with --gpus)."""
    if gpus < 1:
        return f"--gpus must be >= 1 (got {gpus})"
    ws = env.get("WORLD_SIZE")
    if ws is None:
        return "launch" if gpus > 1 else "run"
    if int(ws) != gpus:
        return f"WORLD_SIZE={ws} but --gpus {gpus}"
    return "run"


def launch_cmd(gpus, argv, port):
    """the child command of launch_plan's "launch": torch.distributed.run with
    one process per GPU over 127.0.0.1, re-running this script with the same
    arguments (each child then sees WORLD_SIZE == --gpus)"""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
            f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1", f"--master-port={port}",
            os.path.abspath(__file__)] + list(argv)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def setup_rank(q, rank, world, local_rank):
    """One rank's device and communicators, in this order: the torch process
    group over RCCL on cuda:local_rank (barriers, max-over-ranks, the id
    broadcast), then the library context on the SAME device, then rank 0's
    ncclUniqueId broadcast through torch and the library's own RCCL
    communicator attached with it (qg_ctx_attach_comm).  Returns (dev, dist):
    dist is torch.distributed, or None at world 1."""
    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    dev = q.Device(local_rank)
    if world > 1:
        obj = [q.Device.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(obj, src=0)
        dev.attach_comm(rank, world, obj[0])
    return dev, dist


def main():
    args = parse()
    if args.traffic_probe:
        return traffic_probe(args)
    if args.steps < 1 or args.warmup < 0:
        print("bench.py: --steps must be >= 1 and --warmup >= 0", file=sys.stderr)
        return 2
    full = args.full
    plan = launch_plan(args.gpus, os.environ)
    if plan == "launch":
        # a fresh child per rank, started before this process makes any GPU call
        # (never an exec); this parent only waits and returns the launcher's code
        import subprocess
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        return subprocess.call(launch_cmd(args.gpus, sys.argv[1:], _free_port()), env=env)
    if plan != "run":
        print(f"bench.py: {plan}", file=sys.stderr)
        return 2
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    traffic = None
    if full and world == 1 and not args.no_traffic:
        traffic = measure_traffic(args)  # child processes, before this one touches the GPU
    import quill_amd as q
    dev, dist = setup_rank(q, rank, world, local_rank)
    if dev.world != args.gpus:
        print(f"bench.py: communicator world {dev.world} != --gpus {args.gpus}", file=sys.stderr)
        return 2

    def barrier_sync():
        if dist is not None:
            import torch
            dist.barrier()
            torch.cuda.synchronize()

    def max_over_ranks(x):
        if dist is None:
            return x
        import torch
        t = torch.tensor([x], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())


    n = 1 << args.log_msm
    _progress(rank, f"SRS generation 2^{args.log_msm}")
    t0 = time.perf_counter()
    srs = q.Srs.generate(dev, TAU, n, offset=rank * n)
    scalars = q.DeviceVec(dev, n).fill_random(0x5155494C4C + 2 + rank)
    setup_s = time.perf_counter() - t0

    _progress(rank, "MSM headline")
    dev.trace_marker(LEG_TAGS["msm_2p24"])
    for _ in range(args.warmup):
        srs.msm_dev(scalars)
    dev.enable_timing(True)
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = srs.msm_dev(scalars)
    barrier_sync()
    dt = max_over_ranks(time.perf_counter() - t0)
    ms_per_step = dt / args.steps * 1e3
    value = world * n * args.steps / dt

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, res)
    kern = {}
    for name in ("msm_bucketing", "msm_accumulate", "msm_reduce"):
        ms, cnt = dev.kernel_time(name)
        # a large MSM runs as pieces on two streams (msm.hip msm_device): per-MSM
        # figures sum the pieces' launches; phases of different pieces overlap
        kern[name] = {"ms_avg": ms / max(cnt, 1), "launches": cnt,
                      "ms_per_msm": ms / args.steps, "launches_per_msm": cnt / args.steps}
    dev.enable_timing(False)
    acc_ms = max_over_ranks(kern["msm_accumulate"]["ms_per_msm"])
    achieved = MSM_BYTES_PER_SCALAR * n / (acc_ms * 1e-3) / 1e9
    c_bits, n_win = srs.window_info()

    out = {
        "metric": "G1 MSM scalars/sec at 2^24 + sumcheck-prover ms at 2^20 vars (1/8 GPU)",
        "value": value,
        "unit": "scalars/s",
        "n_gpus": dev.world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u256-montgomery (BN254 Fr scalars, Fq coordinates)",
        "data": "synthetic: SRS [tau^i]g from a fixed tau; uniform Fr scalars (xoshiro256**)",
        "config": {"workload": f"KZG commit / Pippenger G1 MSM, 2^{args.log_msm} BN254 scalars per GPU",
                   "log_msm": args.log_msm, "parallelism": f"msm-shard-by-base-index x{world}",
                   "srs": f"preprocessed once per SRS, outside the timed step: {n_win} "
                          f"window-shifted tables 2^({c_bits}w) P_i (signed {c_bits}-bit digits), "
                          f"128-B rows, {n_win * n * 128 / 1e9:.1f} GB"},
        "roofline": {"bound": "hbm", "kernel": "msm_accumulate", "achieved": achieved,
                     "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                     "traffic": _headline_traffic(traffic),
                     "traffic_row_calibrated": _headline_traffic_row_calibrated(traffic),
                     "traffic_note": "traffic: FETCH_SIZE x2 (the guide's streaming-read "
                                     "correction) + WRITE_SIZE; traffic_row_calibrated: reads "
                                     "rescaled so a calibration kernel's per-lane random 128-B "
                                     "row gathers count 128 B each (pmc._fetch_calibration; "
                                     "the cooperative kernel's whole-row reads need no rescale)",
                     "algorithmic_bytes": MSM_BYTES_PER_SCALAR * n,
                     "note": "MSM is integer-VALU bound (no MFMA form): see compute"},
        "kernels_ms": kern,
        "setup_s": setup_s,
        "commitment_x_low64": hex(0 if res is None else res[0] & ((1 << 64) - 1)),
        # bucket-scan plan copies re-read synchronously (stale generation tag); 0
        # while the event ordering holds
        "msm_plan_refetch": dev.counter("msm_plan_refetch"),
    }

    if full:
        verified = verify_commitment(scalars, res, n, rank, world)
        out["commitment_verified"] = verified["ok"]
        out["commitment_check"] = verified
        fq_peak = dev.microbench_fq_mul()
        # executed: one mixed XYZZ add (8M + 2S = 10 Fq mults) per nonzero digit,
        # W digits per scalar, in msm_accumulate (bucketing/reduce excluded)
        exec_mults = 10 * n_win * n
        out["compute"] = {"fq_mul_per_s_peak_microbench": fq_peak,
                          "survey_fq_mul_equiv_per_scalar": MSM_FQMUL_PER_SCALAR,
                          "survey_equiv_fq_mul_per_s_whole_step":
                              MSM_FQMUL_PER_SCALAR * n / (ms_per_step * 1e-3),
                          "windows": n_win, "window_bits": c_bits,
                          "accumulate_fq_mul_per_s": exec_mults / (acc_ms * 1e-3),
                          "frac": exec_mults / (acc_ms * 1e-3) / fq_peak,
                          "frac_note": "msm_accumulate's executed Fq mults (10 per digit x W "
                                       "digits per scalar) / microbenchmarked Fq-mul peak",
                          "issue_bound_fq_mul_per_s": VMAD_LANE_OPS_PER_S / MADS_PER_FQ_MUL,
                          "frac_issue_bound": exec_mults / (acc_ms * 1e-3)
                          / (VMAD_LANE_OPS_PER_S / MADS_PER_FQ_MUL),
                          "issue_bound_note": "v_mad_u64_u32 lane-ops/s measured with every CU "
                                              "issuing (profiles/r01_isa_rates.json) / 162 partial "
                                              "products per 29-bit Montgomery multiply: a hardware "
                                              "bound, independent of the microbenchmark",
                          "row_gathers_per_s": n_win * n / (acc_ms * 1e-3),
                          "frac_gather_capacity":
                              n_win * n / (acc_ms * 1e-3) / COOP_GATHER_ROWS_PER_S,
                          "gather_note": "random 128-B table rows gathered per second (one per "
                                         "digit) / the chip's measured capacity for whole-row "
                                         "coalesced gathers over a 16 GiB table "
                                         "(micro/gather_bench.hip, profiles/r05_gather_bench.txt)"}
    if traffic is not None:
        out["pmc"] = traffic
    if full:
        run_full_legs(q, dev, args, out, srs, scalars, res, ms_per_step, traffic, barrier_sync,
                      max_over_ranks, rank, world)
    out["msm_plan_refetch"] = dev.counter("msm_plan_refetch")  # over every leg
    # MSM batches whose event-ordered side-stream hand-over the device guard
    # found unordered (recomputed in stream order); 0 while the ordering holds
    out["msm_handover_violation"] = dev.counter("msm_handover_violation")
    if rank == 0:
        if full:
            write_detail(out, args.detail_out)
        print(json.dumps(compact(out), separators=(",", ":")), flush=True)
    srs.close()
    scalars.close()
    dev.close()
    if dist is not None:
        dist.destroy_process_group()


def run_full_legs(q, dev, args, out, srs, scalars, res, ms_per_step, traffic, barrier_sync,
                  max_over_ranks, rank, world):
    """--full: every leg after the headline, each into its own entry of `out`"""
    if not args.no_sumcheck:
        _progress(rank, "sumcheck")
        dev.trace_marker(LEG_TAGS["sumcheck"])
        out["sumcheck"] = bench_sumcheck(q, dev, args, barrier_sync, max_over_ranks, rank)
        if traffic is not None and "error" not in traffic:
            tot = sum((traffic[k]["read_bytes_per_launch"] + traffic[k]["write_bytes_per_launch"])
                      * traffic[k]["launches"] for k in SC_KERNELS if k in traffic)
            out["sumcheck"]["roofline"]["traffic"] = tot
        _progress(rank, "zero-check")
        dev.trace_marker(LEG_TAGS["zerocheck"])
        out["zerocheck"] = bench_zerocheck(q, dev, args, barrier_sync, max_over_ranks, rank)
    if args.log_msm_small > 0:
        _progress(rank, f"MSM 2^{args.log_msm_small} (config 2)")
        dev.trace_marker(LEG_TAGS["msm_2p20"])
        out["msm_2p20"] = bench_msm_small(q, dev, args, barrier_sync, max_over_ranks, rank, world)
    if args.host_input:
        _progress(rank, "MSM from host memory")
        dev.trace_marker(LEG_TAGS["msm_host"])
        out["msm_host_input"] = bench_msm_host(q, dev, args, barrier_sync, max_over_ranks, srs,
                                               scalars, ms_per_step, res)
    if args.oneshot and world == 1:  # a capability leg: one GPU only
        _progress(rank, "MSM over one-shot bases")
        dev.trace_marker(LEG_TAGS["msm_oneshot"])
        out["msm_oneshot"] = bench_msm_oneshot(q, dev, args, barrier_sync, max_over_ranks, srs,
                                               scalars, res)
    if not args.no_scaling_modes:
        _progress(rank, "scaling modes")
        dev.trace_marker(LEG_TAGS["scaling"])
        out["msm_strong_scaling"] = bench_msm_strong(q, dev, args, barrier_sync, max_over_ranks,
                                                     rank, world, srs if world == 1 else None,
                                                     scalars if world == 1 else None)
        if not args.no_sumcheck:
            out["sumcheck_weak_scaling"] = bench_sumcheck(q, dev, args, barrier_sync,
                                                          max_over_ranks, rank, weak=True)
    if args.log_mle > 0:
        _progress(rank, "ML-PCS open")
        dev.trace_marker(LEG_TAGS["mle_open"])
        out["mle_open"] = bench_mle(q, dev, args, barrier_sync, max_over_ranks, rank, world)
    if args.log_logup > 0:
        _progress(rank, "Logup")
        dev.trace_marker(LEG_TAGS["logup"])
        out["logup"] = bench_logup(q, dev, args, barrier_sync, max_over_ranks, rank, world,
                                   traffic)
    if args.log_hp_rows > 0:
        _progress(rank, "HyperPlonk")
        dev.trace_marker(LEG_TAGS["hyperplonk"])
        out["hyperplonk"] = bench_hyperplonk(q, dev, args, barrier_sync, max_over_ranks, rank,
                                             world)
    if rank == 0 and not args.no_cpu_baseline:
        _progress(rank, "CPU baselines")
        dev.trace_marker(LEG_TAGS["cpu_baseline"])
        out["cpu_baseline"] = cpu_baseline(args, srs, scalars)
        if not args.no_sumcheck:
            out["sumcheck"]["cpu_baseline"] = cpu_baseline_sumcheck(args)
        if args.log_mle > 0 and isinstance(out.get("mle_open"), dict):
            out["mle_open"]["cpu_baseline"] = cpu_baseline_mle(args)


# ---------------------------------------------------------------- report
# The driver parses the LAST stdout line, from a bounded tail: the line must stay
# small (round 2's 36 KB line with the per-shape PMC tables was not parsed).
# Everything bulky goes to --detail-out; the line keeps the headline fields,
# roofline, compute, cpu_baseline and one summary per leg.
LINE_MAX_BYTES = 6000
_DROP_KEYS = {"note", "traffic_note", "frac_note", "issue_bound_note", "identity", "pmc",
              "commitment_check", "final_transcript_state", "cpu_model", "metric_note",
              "spans_ms_rank0"}
# sections dropped (in this order) if the line is still over budget
_SHED_ORDER = ("kernels_ms", "sumcheck_weak_scaling", "msm_strong_scaling", "msm_oneshot",
               "zerocheck",
               "msm_host_input",
               "logup", "mle_open", "hyperplonk", "hbm_by_kernel")


def _sig(x, digits=4):
    """floats to `digits` significant digits (JSON bytes, not precision: the
    full values are in --detail-out)"""
    if isinstance(x, bool) or not isinstance(x, float):
        return x
    if x != x or x in (float("inf"), float("-inf")):
        return None
    return float(f"{x:.{digits}g}")


def _shrink(v, depth=0):
    if isinstance(v, dict):
        return {k: _shrink(x, depth + 1) for k, x in v.items()
                if k not in _DROP_KEYS and not k.endswith("_note")}
    if isinstance(v, (list, tuple)):
        return [_shrink(x, depth + 1) for x in v]
    if isinstance(v, str) and len(v) > 160:
        return v[:157] + "..."
    return _sig(v)


def hbm_by_kernel(pmc, top=8):
    """{kernel#leg: [GB/s, fraction of 8 TB/s, avg us]} for the `top` kernels of
    the PMC probe by total time (per probe leg: probe_msm is the headline MSM)"""
    if not isinstance(pmc, dict) or "error" in pmc:
        return None
    sel = "#" if any("#" in k for k in pmc) else None  # older probes: whole-kernel keys
    # the probe's hot-path legs only: not its setup (SRS generation before the
    # first marker, "#pre") nor the FETCH_SIZE calibration launches
    skip_legs = ("#pre", "#probe_cal")
    rows = [(k, d) for k, d in pmc.items()
            if not k.startswith("_") and isinstance(d, dict) and "hbm_gbps" in d
            and (("#" in k and not k.endswith(skip_legs) and not k.startswith(("k_srs_", "k_fb_")))
                 if sel else ("@" not in k))]
    rows.sort(key=lambda kd: -kd[1]["avg_us"] * kd[1].get("launches", 1))
    return {k: [_sig(d["hbm_gbps"], 3), _sig(d["frac_hbm_peak"], 3), _sig(d["avg_us"], 4)]
            for k, d in rows[:top]}


def compact(out, limit=LINE_MAX_BYTES):
    """the stdout line: `out` without notes / PMC tables, floats at 4 digits,
    sections shed in _SHED_ORDER until it fits `limit` bytes"""
    line = _shrink(out)
    hk = hbm_by_kernel(out.get("pmc"))
    if hk:
        line["hbm_by_kernel"] = hk
    if "pmc" in out and isinstance(out["pmc"], dict) and "error" in out["pmc"]:
        line["pmc_error"] = str(out["pmc"]["error"])[:200]
    line["detail"] = out.get("detail_file")
    for key in _SHED_ORDER:
        if len(json.dumps(line, separators=(",", ":"))) <= limit:
            break
        if key in line:
            line[key] = "shed: see detail"
    return line


def dump_outputs(dirname, res):
    """--dump-outputs: what the last timed step returned, the commitment (an
    affine BN254 G1 point), as DIR/commitment.npy: float64[33] = the 16-bit
    little-endian limbs of canonical x (16), of canonical y (16), then the
    infinity flag (limbs 0 when set).  Every entry is an integer below 2^16,
    so float64 holds it exactly."""
    import numpy as np
    x, y = (0, 0) if res is None else res
    limbs = [(v >> (16 * i)) & 0xFFFF for v in (x, y) for i in range(16)]
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, "commitment.npy"),
            np.array(limbs + [1 if res is None else 0], dtype=np.float64))


def write_detail(out, path):
    """the full report (every PMC table and note) as a file; never fatal"""
    if not path:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
        out["detail_file"] = os.path.relpath(path, ROOT)
    except OSError as e:
        out["detail_file"] = f"unwritten: {e}"[:120]


def bench_msm_host(q, dev, args, barrier_sync, max_over_ranks, srs, scalars, resident_ms, res):
    """The drop-in cost of KZG::commit (kzg.rs:61-73): the same 2^log-msm
    commitment with the scalars in pageable host memory (an arkworks `&[Fr]`
    passed to qg_kzg_commit, H2D inside the timed region), next to the
    resident headline; the result must equal the resident commitment."""
    n = 1 << args.log_msm
    arr = scalars.to_numpy()  # (n, 4) Montgomery limbs: arkworks' in-memory Fr
    steps = max(1, min(args.steps, 3))
    got = srs.commit_array(arr, n)
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        got = srs.commit_array(arr, n)
    barrier_sync()
    dt = max_over_ranks(time.perf_counter() - t0)
    ms = dt / steps * 1e3
    return {"ms_per_step": ms, "value": dev.world * n / (ms * 1e-3), "unit": "scalars/s",
            "steps": steps, "input_bytes": 32 * n, "h2d_included_ms": ms - resident_ms,
            "h2d_gbps_effective": 32 * n / ((ms - resident_ms) * 1e-3) / 1e9
            if ms > resident_ms else None,
            "matches_resident_commitment": got == res,
            "note": "pageable host scalars -> qg_kzg_commit; value is never the headline"}


def bench_msm_oneshot(q, dev, args, barrier_sync, max_over_ranks, srs, scalars, res):
    """msm_unchecked (kzg.rs:72) over bases used once: the headline's bases
    uploaded with qg_bases_upload (one table, no window-shifted copies; the MSM
    bins its windows in W passes and adds them by Horner steps) and the
    headline's scalars; the commitment must equal the headline's.  upload_s is
    the whole preprocessing such bases get (the window-shifted tables of
    qg_srs_upload take ~0.65 s at 2^24, profiles/r06m_oneshot_prof.json)."""
    n = 1 << args.log_msm
    xy, inf = srs.download_raw()
    barrier_sync()
    t0 = time.perf_counter()
    one = q.Srs.upload_raw(dev, xy, inf, oneshot=True)
    upload_s = time.perf_counter() - t0
    del xy, inf
    steps = max(1, min(args.steps, 10))
    got = one.msm_dev(scalars)
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        got = one.msm_dev(scalars)
    barrier_sync()
    dt = max_over_ranks(time.perf_counter() - t0)
    c_bits, n_win = one.window_info()
    one.close()
    ms = dt / steps * 1e3
    return {"ms_per_step": ms, "value": dev.world * n / (ms * 1e-3), "unit": "scalars/s",
            "steps": steps, "upload_s": upload_s, "window_bits": c_bits, "windows": n_win,
            "matches_headline_commitment": got == res,
            "note": "qg_bases_upload: one table; value is never the headline"}


def bench_msm_small(q, dev, args, barrier_sync, max_over_ranks, rank, world):
    """BASELINE config 2: Pippenger G1 MSM at 2^k BN254 scalars per GPU
    (kzg.rs:61-73), with an SRS generated for 2^k bases (so the window size is
    the one msm_window_bits picks for 2^k, not the headline's), inputs resident;
    the commitment is checked against the trapdoor identity after the clock."""
    n = 1 << args.log_msm_small
    srs = q.Srs.generate(dev, TAU, n, offset=rank * n)
    scalars = q.DeviceVec(dev, n).fill_random(0x5155494C4C + 20 + rank)
    steps = max(args.steps, 5)
    for _ in range(max(args.warmup, 2)):
        srs.msm_dev(scalars)
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        res = srs.msm_dev(scalars)
    barrier_sync()
    dt = max_over_ranks(time.perf_counter() - t0)
    dev.enable_timing(True)
    for _ in range(steps):
        srs.msm_dev(scalars)
    parts = {nm: dev.kernel_time(nm)[0] / steps
             for nm in ("msm_bucketing", "msm_accumulate", "msm_reduce")}
    dev.enable_timing(False)
    c_bits, n_win = srs.window_info()
    ver = verify_commitment(scalars, res, n, rank, world)
    srs.close()
    scalars.close()
    ms = dt / steps * 1e3
    return {"metric": f"G1 MSM scalars/s at 2^{args.log_msm_small} BN254 scalars per GPU "
                      "(BASELINE config 2)",
            "value": world * n / (ms * 1e-3), "unit": "scalars/s", "ms": ms, "steps": steps,
            "window_bits": c_bits, "windows": n_win, "parts_ms": parts,
            "commitment_verified": ver["ok"], "scaling": "weak"}


def bench_msm_strong(q, dev, args, barrier_sync, max_over_ranks, rank, world, srs=None,
                     scalars=None):
    """Strong-scaling MSM: ONE commitment to a degree 2^log-msm polynomial split
    over the ranks (rank r owns bases/scalars [r n/N, (r+1) n/N)); value = n /
    max-over-ranks time.  At N = 1 it reuses the headline SRS and scalars."""
    n = 1 << args.log_msm
    L = n // world
    own = srs is None
    if own:
        srs = q.Srs.generate(dev, TAU, L, offset=rank * L)
        scalars = q.DeviceVec(dev, L).fill_random(0x5155494C4C + 6 + rank)
    steps = max(1, min(args.steps, 3))
    srs.msm_dev(scalars, L)
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        srs.msm_dev(scalars, L)
    barrier_sync()
    dt = max_over_ranks(time.perf_counter() - t0)
    if own:
        srs.close()
        scalars.close()
    return {"metric": f"G1 MSM scalars/s, one 2^{args.log_msm} commitment split over the GPUs",
            "value": n * steps / dt, "unit": "scalars/s", "ms_per_step": dt / steps * 1e3,
            "steps": steps, "scaling": "strong", "per_rank_scalars": L}


def bench_sumcheck(q, dev, args, barrier_sync, max_over_ranks, rank, weak=False):
    from quill_amd.hyperplonk import VirtualPolyExpr as E, sumcheck_prove_device
    world = dev.world
    lw = max(world.bit_length() - 1, 0)
    # strong: one 2^n prove sharded by the high index bits; weak: 2^n entries per
    # GPU (a 2^(n + log2 N)-variable prove)
    nv = args.log_sumcheck + (lw if weak else 0)
    N = (1 << nv) // world  # this rank's block of every table (sharded by the high bits)
    tabs = [q.DeviceVec(dev, N).fill_random(0x5155494C4C + 3 + 7 * i + 100 * rank) for i in range(3)]
    expr = E.Input(0) * E.Input(1) * E.Input(2)
    claimed = 0  # the prover is deterministic in its inputs; the claim is absorbed as-is
    for _ in range(args.warmup):
        sumcheck_prove_device(dev, nv, tabs, expr, claimed, q.Transcript(b"sumcheck_bench"))
    # the timed calls run without the library's kernel-timing events (they add
    # ~25 us per call of event records to the prover); a second pass with the
    # events on gives the per-kernel split
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sumcheck_prove_device(dev, nv, tabs, expr, claimed, q.Transcript(b"sumcheck_bench"))
    barrier_sync()
    dt = max_over_ranks(time.perf_counter() - t0)
    ms = dt / args.steps * 1e3
    dev.enable_timing(True)
    barrier_sync()
    t1 = time.perf_counter()
    for _ in range(args.steps):
        sumcheck_prove_device(dev, nv, tabs, expr, claimed, q.Transcript(b"sumcheck_bench"))
    barrier_sync()
    ms_timed = max_over_ranks(time.perf_counter() - t1) / args.steps * 1e3
    rk_ms, rk_n = dev.kernel_time("sumcheck_round")
    tl_ms, tl_n = dev.kernel_time("sumcheck_tail")
    dev.enable_timing(False)
    for t in tabs:
        t.close()
    # algorithmic bytes.  SURVEY §8(d): round j reads k*32*2^(n-j) B and writes
    # half that, 96 k 2^n B in all (302 MB at k = 3, n = 20).  This prover never
    # writes round 0's folded tables (round 1's kernel folds while it reads the
    # inputs), so its own rule drops that write: 251.7 MB.  `frac` uses the
    # prover's rule; `frac_survey_rule` the §8(d) total.
    k = 3
    NG = 1 << nv
    total_bytes = sum(k * 32 * (NG >> j) + (k * 32 * (NG >> j) // 2 if j > 0 else 0)
                      for j in range(nv))
    survey_bytes = 96 * k * NG
    per_call_gbps = total_bytes / (ms * 1e-3) / 1e9
    return {"metric": f"sumcheck-prover ms at 2^{nv} vars (h = g1*g2*g3, degree 3)",
            "ms": ms, "higher_is_better": False,
            "roofline": {"bound": "hbm", "kernel": "sumcheck prove (all rounds)",
                         "achieved": per_call_gbps, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                         "frac": per_call_gbps / HBM_PEAK_GBPS, "traffic": None,
                         "algorithmic_bytes": total_bytes,
                         "bytes_rule": "SURVEY 8(d) per-round reads + writes, minus round 0's "
                                       "write (folded into round 1's read)",
                         "survey_bytes": survey_bytes,
                         "frac_survey_rule": survey_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS},
            "parallelism": (f"sharded x{world} ({'weak' if weak else 'strong'} scaling)"
                            if world > 1 else "single GPU"),
            "scaling": "weak" if weak else "strong",
            "round_kernels_ms_per_call": rk_ms / max(args.steps, 1),
            "tail_kernel_ms_per_call": tl_ms / max(args.steps, 1),
            "ms_with_kernel_timing": ms_timed}


def bench_zerocheck(q, dev, args, barrier_sync, max_over_ranks, rank):
    """SURVEY 8(d) C3's variant: ZeroCheckProof::prove (zerocheck.rs:14-49) at
    2^log-sumcheck variables, h = g1*g2 - g3 (k = 4 tables with eq, degree 3 after
    x eq): z drawn, eq(., z) built on the device, the sumcheck of h*eq.  Sharded
    like the sumcheck leg (strong: one 2^n prove over the ranks)."""
    from quill_amd import VirtualPolyExpr as E
    from quill_amd.hyperplonk import zerocheck_prove_device
    world = dev.world
    nv = args.log_sumcheck
    N = (1 << nv) // world
    tabs = [q.DeviceVec(dev, N).fill_random(0x5155494C4C + 13 + 7 * i + 100 * rank)
            for i in range(3)]
    expr = E.Input(0) * E.Input(1) - E.Input(2)
    for _ in range(args.warmup):
        zerocheck_prove_device(dev, nv, tabs, expr, q.Transcript(b"zerocheck_bench"))
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        zerocheck_prove_device(dev, nv, tabs, expr, q.Transcript(b"zerocheck_bench"))
    barrier_sync()
    ms = max_over_ranks(time.perf_counter() - t0) / args.steps * 1e3
    for t in tabs:
        t.close()
    return {"metric": f"zero-check prover ms at 2^{nv} vars (h = g1*g2 - g3, x eq)", "ms": ms,
            "higher_is_better": False,
            "parallelism": f"sharded x{world} (strong scaling)" if world > 1 else "single GPU",
            "note": "random tables (the prover's work does not depend on h vanishing); "
                    "includes the eq table and the z draws"}


def bench_mle(q, dev, args, barrier_sync, max_over_ranks, rank=0, world=1):
    """Config C4: MultilinearPCS commit + open (MLEvalProof::prove) at 2^k
    evaluations, point drawn from the transcript after absorbing the commitment
    (the mlpcs.rs:258-267 pattern).  With N ranks the 2^k evaluations and the SRS
    are sharded (rank r holds [r 2^k/N, (r+1) 2^k/N)): eq/dot/quotients and all
    six MSMs sharded, the S polynomial split by frequency residue (strong scaling)."""
    from quill_amd import KZG, Transcript
    k = args.log_mle
    n = 1 << k
    L = n // world
    kzg = KZG(dev, q.Srs.generate(dev, TAU, L, offset=rank * L), n - 1)
    poly = q.DeviceVec(dev, L).fill_random(0x5155494C4C + 4 + 1000 * rank)

    def step():
        C = kzg.srs.msm_dev(poly)
        t = Transcript(b"MLPCS bench")
        t.append_g1(C)
        point = [t.draw_field_element() for _ in range(k)]
        return kzg.open_dev(poly, L, point, t)

    for _ in range(max(1, args.warmup)):
        step()
    names = ("eq_table", "inner_product", "s_polynomial", "kzg_division", "msm_bucketing",
             "msm_bucketing_side", "msm_accumulate", "msm_reduce")
    steps = max(1, min(args.steps, 3))
    # timed steps without the library's phase-timing events; one more step
    # with them gives the phase split
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    barrier_sync()
    dt = max_over_ranks(time.perf_counter() - t0)
    dev.enable_timing(True)
    t1 = time.perf_counter()
    step()
    ms_timed = (time.perf_counter() - t1) * 1e3
    # additive device-busy split (overlapped intervals shared evenly: the parts
    # sum to the busy time); the per-stream spans overlap and stay apart
    parts = dev.phase_split(names)
    spans = {nm: dev.kernel_time(nm)[0] for nm in names}
    dev.enable_timing(False)
    poly.close()
    kzg.srs.close()
    return {"metric": f"ML-PCS commit + open (MLEvalProof::prove) ms at 2^{k} evaluations",
            "ms": dt / steps * 1e3, "higher_is_better": False, "msms_per_step": 6,
            "parts_ms_rank0": parts, "spans_ms_rank0": spans,
            "ms_with_phase_timing": ms_timed, "steps": steps,
            "sharding": f"2^{k} evaluations over {world} rank(s) (strong scaling); "
                        "S polynomial split by frequency residue (one all-to-all)",
            "note": "6 MSMs (commit, S commitment, 4 KZG quotients) dominate"}


LOGUP_A, LOGUP_BETA = 0xA1FA, 0xBE7A5EED


def bench_logup(q, dev, args, barrier_sync, max_over_ranks, rank=0, world=1, traffic=None):
    """Logup log-derivative column (multiset_check.rs:43-95 / set_inclusion.rs:
    93-131, subset mode): out = m / (beta + h) with h = t0 + a t1 (two batched
    columns, lookup.rs:46-56) and m = t2, 2^k rows per GPU (weak scaling)."""
    from quill_amd import VirtualPolyExpr as E
    from quill_amd.logup import logup_column_device
    k = args.log_logup
    n = 1 << k
    lw = max(world.bit_length() - 1, 0)
    tabs = [q.DeviceVec(dev, n).fill_random(0x5155494C4C + 5 + 11 * i + 100 * rank)
            for i in range(3)]
    out = q.DeviceVec(dev, n)
    h = E.Input(0) + E.Const(LOGUP_A) * E.Input(1)
    m = E.Input(2)
    for _ in range(max(1, args.warmup)):
        logup_column_device(dev, k + lw, tabs, h, LOGUP_BETA, out, m)
    # wall time without the library's kernel-timing events, then the same
    # calls with them for the kernel time
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        s = logup_column_device(dev, k + lw, tabs, h, LOGUP_BETA, out, m)
    barrier_sync()
    dt = max_over_ranks(time.perf_counter() - t0)
    dev.enable_timing(True)
    for _ in range(args.steps):
        logup_column_device(dev, k + lw, tabs, h, LOGUP_BETA, out, m)
    kms, kn = dev.kernel_time("logup_column")
    dev.enable_timing(False)
    # device time per column: denominators + block scan, then the inverses (the
    # host's single finv in between is outside the timed regions); with
    # QG_LOGUP_FUSED=1 the one-pass kernel + the block-sum kernel
    kern_ms = max_over_ranks(kms / max(args.steps, 1))
    nbytes = LOGUP_BYTES_PER_ROW * n
    lg_kernels = ("k_logup_fused", "k_logup_den", "k_logup")
    lg_traffic = [_kernel_traffic(traffic, k) for k in lg_kernels]
    fused = os.environ.get("QG_LOGUP_FUSED", "0") != "0"
    res = {"metric": f"Logup column rows/s at 2^{k} rows per GPU (m / (beta + t0 + a t1))",
           "value": world * n * args.steps / dt, "unit": "rows/s", "higher_is_better": True,
           "ms": dt / args.steps * 1e3, "kernel_ms": kern_ms,
           "roofline": {"bound": "hbm", "kernel": "logup_column", "achieved":
                        nbytes / (kern_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                        "frac": nbytes / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS,
                        "traffic": (None if all(t is None for t in lg_traffic) else
                                    sum(t or 0 for t in lg_traffic)),
                        "algorithmic_bytes": nbytes,
                        "note": ("3 table reads + 1 column write of 32 B per row, one pass "
                                 "(a binary-GCD inversion per 2048-row block)" if fused else
                                 "3 table reads + 1 column write of 32 B per row; the kernels "
                                 "also write and re-read the denominators (+64 B/row)")},
           "column_sum_low64": hex(s & ((1 << 64) - 1))}
    if not fused:
        # the column is multiply-bound: Montgomery products per row of the
        # 3-kernel path, counted from csrc/logup.hip (denominator a t1 and the
        # block product 2 + scans 0.5; prefix 0.875, wave scans 1.5, wave / block
        # inverses 1.0, back-substitution 1.75, multiplier 1)
        muls = LOGUP_MULS_PER_ROW * n
        res["compute"] = {"fr_mul_per_row": LOGUP_MULS_PER_ROW,
                          "fr_mul_per_s": muls / (kern_ms * 1e-3),
                          "frac_issue_bound": muls / (kern_ms * 1e-3)
                          / (VMAD_LANE_OPS_PER_S / MADS_PER_FQ_MUL)}
    if rank == 0 and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline_logup(args, tabs, out)
    for t in tabs + [out]:
        t.close()
    return res


LOGUP_MULS_PER_ROW = 8.6

# msm_bucketing_side: the bucketing of the MSMs of a batch, which run on two
# side streams by parity.  parts_ms_rank0 is the additive device-busy split
# (qg_ctx_phase_split: an interval where several phases run, on any stream, is
# shared evenly among them, so the parts sum to the busy time <= the proof
# time); spans_ms_rank0 keeps the per-stream spans, which overlap
HP_PHASES = ("msm_bucketing", "msm_bucketing_side", "msm_accumulate", "msm_reduce",
             "sumcheck_round", "sumcheck_tail", "logup_column", "eq_table", "inner_product",
             "s_polynomial", "kzg_division")


def bench_hyperplonk(q, dev, args, barrier_sync, max_over_ranks, rank=0, world=1):
    """Config C5: HyperPlonk::prove (hyperplonk/src/proof/proof.rs:239-301) over
    the reference's two test circuits (test_basic_proof.rs:17-105) scaled to
    2^k rows: fibonacci (4 columns, trace 2^(k+2)) + modified fibonacci (5 -> 8
    columns, trace 2^(k+3)); SRS max_degree 2^(k+3).  The witnesses are resident
    in HBM before the timed region; constraint checks, commitments, zero-checks,
    permutation checks and all ML-PCS openings are inside it.  With N ranks the
    proof is sharded (the transcript orders the traces, the work
    inside each step shards): rank r holds the row block r of every column
    (resident before timing); the full-witness exchange, every MSM, sumcheck,
    Logup column and opening run sharded; every rank outputs the same proof
    (strong scaling; proofs/s = 1 / time)."""
    from quill_amd import KZG, HyperPlonk, TraceWitness
    from quill_amd import examples as ex
    k = args.log_hp_rows
    rows = 1 << k
    t0 = time.perf_counter()
    cws = [ex.fibonacci_circuit_and_trace(rows), ex.modified_fibonacci_circuit_and_trace(rows)]
    maxdeg = max(c.num_cols() * c.num_rows() for c, _ in cws)
    pcs = KZG.trusted_setup(maxdeg, TAU, dev)
    hp = HyperPlonk.preprocess([c for c, _ in cws], pcs)
    wits, resident = [], []
    RL = rows // world
    for c, w in cws:
        # single GPU: the full witness; sharded: this rank's row block of each column
        buf = q.DeviceVec(dev, RL * c.num_cols())
        resident.append(buf)
        for i, col in enumerate(w):
            q.DeviceVec.from_canonical(dev, col[rank * RL:(rank + 1) * RL], out=buf,
                                       offset=i * RL)
        wits.append(TraceWitness.from_full(buf, c.num_cols()) if world == 1 else
                    TraceWitness([buf.view(i * RL, RL) for i in range(c.num_cols())]))
    del cws
    setup_s = time.perf_counter() - t0
    for _ in range(max(1, min(args.warmup, 1))):
        proof = hp.prove(pcs, wits)
    steps = max(1, min(args.steps, 2))
    # the timed proofs run without the library's phase-timing events (~1100
    # event records per proof); one more proof with them gives the phase split
    barrier_sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        proof = hp.prove(pcs, wits)
    barrier_sync()
    dt = max_over_ranks(time.perf_counter() - t0)
    dev.enable_timing(True)
    barrier_sync()
    t1 = time.perf_counter()
    proof = hp.prove(pcs, wits)
    barrier_sync()
    ms_timed = max_over_ranks(time.perf_counter() - t1) * 1e3
    parts = dev.phase_split(HP_PHASES)
    spans = {nm: dev.kernel_time(nm)[0] for nm in HP_PHASES}
    dev.enable_timing(False)
    nopen = sum(len(tp.openings_zero_check) + len(tp.openings_public) + 5
                for tp in proof.trace_proofs)
    res = {"metric": f"HyperPlonk prove ms, fibonacci + modified-fibonacci traces at 2^{k} rows "
                     f"(2^{k + 2} + 2^{k + 3} cells)",
           "ms": dt / steps * 1e3, "higher_is_better": False,
           "proofs_per_s": steps / dt, "steps": steps, "setup_s": setup_s,
           "ml_openings_per_proof": nopen, "parts_ms_rank0": parts,
           "parts_sum_ms": sum(parts.values()), "spans_ms_rank0": spans,
           "ms_with_phase_timing": ms_timed,
           "final_transcript_state": hp.last_transcript.state.hex(),
           "parallelism": f"sharded x{world}" if world > 1 else "single GPU",
           "scaling": "strong"}
    if rank == 0 and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline_hyperplonk(args)
    for b in resident:
        b.close()
    for pk in hp.trace_pks:
        for v in [pk.id_poly, pk.permutation_poly] + pk.public_values + pk.public_rows:
            v.close()
    pcs.close()
    return res


def cpu_baseline_hyperplonk(args):
    """HyperPlonk::prove (proof.rs:145-301) with the reference's data flow in C
    (oracle/hyperplonk_c.py: Pippenger commitments, MLEvalProof::prove, the
    reference-structured sumchecks, Logup columns, eq tables), orchestrated by
    the Python restatement and bit-exact with it (tests/test_oracle_c.py), on
    the same two circuits at 2^k rows; single thread; linear extrapolation."""
    try:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import hyperplonk_c as hc
        import hyperplonk_oracle as ho
        import quill_oracle as qo
    except Exception as e:
        return {"ms": None, "error": f"oracle unavailable: {e}"}
    lg = args.cpu_hp_rows_log
    rows = 1 << lg
    c1, w1 = ho.fibonacci_circuit_and_trace(rows)
    c2, w2 = ho.modified_fibonacci_circuit_and_trace(rows)
    pcs = qo.KZG(max(c1.num_cols(), c2.num_cols()) * rows, TAU)
    hp = ho.HyperPlonk.preprocess([c1, c2], pcs)
    with hc.c_backend(TAU, pcs.max_degree + 1):
        t0 = time.perf_counter()
        hp.prove(pcs, [w1, w2])
        sec = time.perf_counter() - t0
    scale = 1 << max(args.log_hp_rows - lg, 0)
    return {"ms_sample": sec * 1e3, "sample_log_rows": lg, "ms_extrapolated": sec * 1e3 * scale,
            "cores": 1, "kind": "port",
            "sample": f"HyperPlonk::prove at 2^{lg} rows (fib 2^{lg + 2} + mod-fib 2^{lg + 3} "
                      f"cells), heavy steps in C with the reference's data flow, Python "
                      f"orchestration in the timed region; x{scale} (MSM/FFT-dominated, slightly "
                      f"super-linear) estimates 2^{args.log_hp_rows} rows"}


def cpu_baseline_logup(args, tabs, out):
    """The reference's per-row loop (evaluate h, .inverse(), * m) restated in C
    (oracle/oracle_c.c: oc_logup_column, ark-ff binary-Euclid inverse), single
    thread, on the first 2^18 rows of the timed workload; must equal the GPU
    column on those rows."""
    try:
        oc = _oracle_c()
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import quill_oracle as qo
    except Exception as e:
        return {"value": None, "unit": "rows/s", "error": f"oracle C library unavailable: {e}"}
    ns = min(1 << 18, len(out))
    cols = [t.to_numpy(ns) for t in tabs]
    ref, sec = oc.logup_column_arrays(cols[0], cols[1], cols[2], qo.fr_to_limbs_mont(LOGUP_A),
                                      qo.fr_to_limbs_mont(LOGUP_BETA))
    import numpy as np
    return {"value": ns / sec, "unit": "rows/s", "cores": 1, "kind": "port",
            "sample": f"first {ns} rows of the timed workload, per-row inverse like the "
                      f"reference ({sec:.2f} s)", "seconds": sec,
            "matches_gpu_column_of_sample": bool(np.array_equal(ref, out.to_numpy(ns)))}


def _kernel_traffic(traffic, kernel, grid=None):
    """HBM bytes per launch (PMC, corrected) or None; with `grid`, of the launches
    of that shape (kernel@grid work-items) only"""
    key = kernel if grid is None else f"{kernel}@{grid}"
    if not traffic or "error" in traffic or key not in traffic:
        return None
    d = traffic[key]
    return d["read_bytes_per_launch"] + d["write_bytes_per_launch"]


# the bucket-accumulation kernels, the headline's first: k_msm_accumulate_coop
# (wave-cooperative row gathers, 2^25+ entries), k_msm_accumulate (per-lane)
ACC_KERNELS = ("k_msm_accumulate_coop", "k_msm_accumulate")


def _headline_acc(traffic):
    """(kernel, PMC row) of the probe's headline-MSM accumulate: by its leg
    marker, else the largest launch shape (the 2^log-msm MSM runs first)"""
    for k in ACC_KERNELS:
        leg = traffic.get(f"{k}#probe_msm")
        if leg and "read_bytes_per_launch" in leg:
            return k, leg
    for k in ACC_KERNELS:
        shapes = [x for x in traffic if x.startswith(f"{k}@")]
        if shapes:
            return k, traffic[max(shapes, key=lambda x: int(x.split("@")[1]))]
    for k in ACC_KERNELS:
        if k in traffic and "read_bytes_per_launch" in traffic[k]:
            return k, traffic[k]
    return None, None


def _headline_traffic(traffic):
    """PMC bytes per headline MSM of its accumulate (every launch of the probe's
    headline leg / shape belongs to that MSM's pieces)"""
    if not traffic or "error" in traffic:
        return None
    _, d = _headline_acc(traffic)
    if d is None:
        return None
    return (d["read_bytes_per_launch"] + d["write_bytes_per_launch"]) * max(d.get("launches", 1), 1)


def _headline_traffic_row_calibrated(traffic):
    """the same bytes with the read side scaled by the row-gather calibration
    (pmc_traffic.py CAL_*): per-lane random 128-B row gathers (five 16-B loads)
    counted at 128 B each; the cooperative kernel reads whole 128-B rows in
    coalesced requests, which FETCH_SIZE counts as they are (no rescaling)"""
    cal = (traffic or {}).get("_fetch_calibration")
    if not cal or "error" in traffic:
        return None
    k, d = _headline_acc(traffic)
    if d is None:
        return None
    f = 1.0 if k == "k_msm_accumulate_coop" else cal["gather_read_factor"]
    return ((d["read_bytes_per_launch"] * f + d["write_bytes_per_launch"])
            * max(d.get("launches", 1), 1))


def _oracle_c():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_c
    oracle_c.lib()
    return oracle_c


def verify_commitment(scalars, res, n, rank, world):
    """Checker of the timed headline result (the oracle's C restatement, test
    infrastructure; never on the measured path): the commitment equals the
    trapdoor identity [sum_r tau^(r n) sum_i s_i tau^i] g (kzg.rs:44-47, 61-73),
    each rank's Horner over its own downloaded scalars, outside the timed region."""
    t0 = time.perf_counter()
    try:
        oc = _oracle_c()
        v = oc.fr_horner(scalars.to_numpy(), TAU) * pow(TAU, rank * n, oc.R_MOD) % oc.R_MOD
        err = None
    except Exception as e:  # the checker is missing: report, never substitute
        v, err = None, str(e)[-300:]
    vs = [v]
    if world > 1:
        import torch.distributed as tdist
        vs = [None] * world
        tdist.all_gather_object(vs, v)
    if any(x is None for x in vs):
        return {"ok": None, "error": err or "a rank could not run the checker"}
    total = sum(vs) % oc.R_MOD
    ok = oc.g1_mul((1, 2), total) == res
    return {"ok": bool(ok), "identity": "C == [sum_i s_i tau^i] g (trapdoor, oracle C Horner)",
            "seconds": time.perf_counter() - t0}


def cpu_baseline(args, srs, scalars):
    """Oracle C restatement of arkworks' single-thread Pippenger (oracle/_build),
    on a prefix of this run's own SRS and scalars; the GPU MSM of the same
    prefix must give the same point."""
    try:
        oc = _oracle_c()
    except Exception as e:  # the checker is missing: report, do not substitute
        return {"value": None, "unit": "scalars/s", "error": f"oracle C library unavailable: {e}"}
    ns = min(1 << args.cpu_sample_log, len(srs))
    xy, inf = srs.download_raw(0, ns)
    sc = scalars.to_numpy(ns)
    tm, tc, (cxy, cinf) = oc.bench_msm_arrays(xy, inf, sc)
    nth = oc.usable_cores()
    tmt, (mxy, minf) = oc.bench_msm_arrays_mt(xy, inf, sc, nth)
    from quill_amd.field import g1_from_abi
    gpu = srs.msm_dev(scalars, ns)
    all_cores = {"value": ns / tmt, "unit": "scalars/s", "cores": nth, "kind": "port",
                 "sample": f"same 2^{args.cpu_sample_log} sample, ark-ec's parallel window "
                           f"split on {nth} threads ({tmt:.2f} s); the reference builds "
                           "without rayon, so this is an all-cores port",
                 "seconds": tmt, "matches_gpu_msm_of_sample": g1_from_abi(mxy, minf) == gpu}
    return {"value": ns / tm, "unit": "scalars/s", "cores": 1, "kind": "port",
            "all_cores": all_cores,
            "sample": f"the first 2^{args.cpu_sample_log} bases and scalars of the timed "
                      f"workload, one msm_unchecked ({tm:.2f} s, single thread like the "
                      f"reference); KZG::commit as written (+ into_affine of every SRS point) "
                      f"{ns / tc:.4g} scalars/s",
            "seconds": tm, "kzg_commit_as_written_scalars_per_s": ns / tc,
            "matches_gpu_msm_of_sample": g1_from_abi(cxy, cinf) == gpu,
            "cpu_model": oc.cpu_model()}


def cpu_baseline_mle(args):
    """C restatement of MLEvalProof::prove with the reference's data flow
    (compute_pr by domain evaluation + IFFT, ark-poly FFT products in the S
    polynomial, long division + the FFT assert per quotient, single-thread
    Pippenger for the six MSMs) on a bounded 2^(n-5) sample, checked bit-exact
    against the Python oracle in tests/test_oracle_c.py; linear extrapolation."""
    try:
        oc = _oracle_c()
    except Exception as e:
        return {"ms": None, "error": f"oracle C library unavailable: {e}"}
    ls = max(args.log_mle - 5, 1)
    sec = oc.bench_mle_open_ref(ls)
    return {"ms_sample": sec * 1e3, "sample_log_evals": ls,
            "ms_extrapolated": sec * 1e3 * (1 << (args.log_mle - ls)), "cores": 1,
            "kind": "port",
            "note": f"MLEvalProof::prove (mlpcs.rs:83-124) restated in C at 2^{ls} evaluations "
                    f"(the prove only; SRS generated before the clock); x{1 << (args.log_mle - ls)}"
                    f" (MSM- and FFT-dominated, slightly super-linear) estimates 2^{args.log_mle}"}


def cpu_baseline_sumcheck(args):
    """Evaluation-form C prover at the bench size (1 thread, a lower bound on the
    reference), the reference-structured C prover (per-pair DensePolynomials,
    FFT products, clones: sumcheck.rs:28-114, virtual_polynomial.rs:300-320) on
    a bounded 2^(n-2) sample with the linear extrapolation to 2^n, and the
    evaluation form on all usable cores at 2^n."""
    try:
        oc = _oracle_c()
    except Exception as e:
        return {"ms": None, "error": f"oracle C library unavailable: {e}"}
    out = oc.bench_sumcheck_baseline(args.log_sumcheck)
    ls = max(args.log_sumcheck - 2, 1)
    t_ref = oc.bench_sumcheck_ref(ls)
    out["reference_structured"] = {
        "ms_sample": t_ref * 1e3, "sample_log_vars": ls,
        "ms_extrapolated": t_ref * 1e3 * (1 << (args.log_sumcheck - ls)), "cores": 1,
        "kind": "port",
        "note": f"the reference's data flow restated in C at 2^{ls} vars; work is linear in "
                f"2^n, so x{1 << (args.log_sumcheck - ls)} gives the 2^{args.log_sumcheck} "
                "estimate"}
    nth = oc.usable_cores()
    out["all_cores"] = {"ms": oc.bench_sumcheck_mt(args.log_sumcheck, nth) * 1e3, "cores": nth,
                        "kind": "port", "sample": f"evaluation form, 2^{args.log_sumcheck} vars"}
    return out


if __name__ == "__main__":
    sys.exit(main() or 0)
