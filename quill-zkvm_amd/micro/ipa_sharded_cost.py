"""Costs of the sharded inner-product argument (qg_ipa_prove_dev with a
communicator), one part per run.  Ranks are host threads over the loopback
communicator SHARING ONE GPU, so every figure here is contended (the ranks'
kernels interleave and a collective waits for the slowest rank): not multi-GPU
figures.

  --part presum   the "s_presum" region (HIP events) of one sharded IPA call at
                  2^22 global coefficients, world 4: the fused k_s_presum_fg
                  launch against k_s_presum launched per operand and residue
                  (QG_S_PRESUM_FUSED=0), cases interleaved call by call
  --part ipa      per-rank wall time and additive device-busy split of the
                  sharded IPA at 2^20 global coefficients, world 2 and 4
  --part open     a single sharded ML opening (qg_mle_open_dev) at 2^20
                  evaluations, world 2 and 4, rank 0's median wall time of 7
                  calls, on the library QG_LIB names: run on the parent's build
                  and on this one, alternating, to see that it did not move
  --merge a.json ...   one object from the parts' outputs (--out writes it)

  QG_LIB=<libquill_gpu.so> python quill-zkvm_amd/micro/ipa_sharded_cost.py
      --part <p> [--inner 5] [--outer 5] [--out f.json]
Medians of --inner calls, repeated --outer times; `spread` is max - min of the
repeated medians."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
if os.environ.get("QG_LIB"):  # A/B builds of the library (micro benchmark only)
    import quill_amd._lib as _L
    _L.LIB_PATH = os.path.abspath(os.environ["QG_LIB"])
    import ctypes
    _old = ctypes.CDLL(_L.LIB_PATH)  # an older build lacks the newer entries: not bound
    for _k in [k for k in _L.PROTOTYPES if not hasattr(_old, k)]:
        del _L.PROTOTYPES[_k]

TAU = 0x5155494C4C5F54415521
PHASES = ("inner_product", "s_polynomial", "kzg_division", "kzg_open_check", "msm_bucketing",
          "msm_bucketing_side", "msm_accumulate", "msm_reduce")
NOTE = ("loopback ranks are host threads sharing one GPU: contended figures, not multi-GPU "
        "figures; every exchange includes the wait for the slowest rank")


def summary(medians):
    return {"medians": medians, "median": statistics.median(medians),
            "spread": max(medians) - min(medians)}


def run_ranks(world, fn):
    import quill_amd as q
    group = q.Device.loopback_group(world)
    out, err = [None] * world, []

    def body(rank):
        try:
            dev = q.Device(0)
            dev.attach_loopback(group, rank)
            out[rank] = fn(dev, rank, world)
            dev.close()
        except Exception as e:
            err.append(e)
    ths = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    q.lib().qg_loopback_destroy(group)
    if err:
        raise err[0]
    return out


def ipa_setup(q, dev, rank, L, M):
    kzg = q.KZG(dev, q.Srs.generate(dev, TAU, L, offset=rank * L), M - 1)
    f = q.DeviceVec(dev, L).fill_random(0x495041 + rank)
    g = q.DeviceVec(dev, L).fill_random(0x495042 + rank)

    def step():
        t = q.Transcript(b"IPA sharded bench")
        return q.InnerProductProof.prove(f, g, kzg, t), t.state
    return step


def part_presum(args):
    """every rank sets the switch to the same value before the same call, and no
    rank leaves a call before all have passed its pre-sum (the all-to-all comes
    after it), so the process-wide variable is read as set"""
    import quill_amd as q
    world, M = 4, 1 << args.log
    L = M // world

    def fn(dev, rank, world):
        step = ipa_setup(q, dev, rank, L, M)

        def case(v):
            os.environ["QG_S_PRESUM_FUSED"] = v
            return step()
        for _ in range(2):
            assert case("1") == case("0")
        meds = {"fused": [], "four_launches": []}
        for _ in range(args.outer):
            vals = {k: [] for k in meds}
            for _ in range(args.inner):
                for name, v in (("fused", "1"), ("four_launches", "0")):
                    dev.enable_timing(True)
                    case(v)
                    vals[name].append(dev.kernel_time("s_presum")[0])
            for k in meds:
                meds[k].append(statistics.median(vals[k]))
        dev.enable_timing(False)
        return {k: summary(m) for k, m in meds.items()}
    ranks = run_ranks(world, fn)
    os.environ.pop("QG_S_PRESUM_FUSED", None)
    res = {"global_coefficients": M, "world": world, "inner": args.inner, "outer": args.outer,
           "region": "s_presum (HIP events), ms per call", "note": NOTE, "ranks": ranks}
    # ranks 1 and 3 own a residue with c != -c (four outputs); 0 and 2 have two
    for name, rs in (("four_outputs", (1, 3)), ("two_outputs", (0, 2))):
        fu = statistics.median(ranks[r]["fused"]["median"] for r in rs)
        fo = statistics.median(ranks[r]["four_launches"]["median"] for r in rs)
        noise = max(max(ranks[r][k]["spread"] for k in ("fused", "four_launches")) for r in rs)
        d = fu - fo
        res[name] = {"fused_ms": fu, "launch_per_output_ms": fo, "fused_minus_launches": d,
                     "noise": noise,
                     "faster": ("launches" if d > 0 else "fused") if abs(d) > noise
                     else "within noise"}
    return res


def part_ipa(args):
    import quill_amd as q
    M = 1 << args.log
    res = {"global_coefficients": M, "inner": args.inner, "outer": args.outer, "note": NOTE}
    for world in (2, 4):
        L = M // world

        def fn(dev, rank, world, L=L):
            step = ipa_setup(q, dev, rank, L, M)
            for _ in range(2):
                step()
            meds = []
            for _ in range(args.outer):
                v = []
                for _ in range(args.inner):
                    t0 = time.perf_counter()
                    step()
                    v.append((time.perf_counter() - t0) * 1e3)
                meds.append(statistics.median(v))
            dev.enable_timing(True)
            step()
            parts = dev.phase_split(PHASES)
            dev.enable_timing(False)
            return {"wall_ms": summary(meds), "parts_ms": {**parts, "sum": sum(parts.values())},
                    "open_check_failures": dev.counter("open_check_failures")}
        res[f"world_{world}"] = {"coefficients_per_rank": L, "ranks": run_ranks(world, fn)}
    return res


def part_open(args):
    import quill_amd as q
    nv = args.log
    N = 1 << nv
    t0 = q.Transcript(b"point")
    point = [t0.draw_field_element() for _ in range(nv)]
    res = {"evaluations": N, "calls": 7, "library": os.environ.get("QG_LIB", "in-tree"),
           "note": NOTE}
    for world in (2, 4):
        L = N // world

        def fn(dev, rank, world, L=L):
            kzg = q.KZG(dev, q.Srs.generate(dev, TAU, L, offset=rank * L), N - 1)
            v = q.DeviceVec(dev, L).fill_random(0x4F50 + rank)

            def step():
                t = q.Transcript(b"sharded open bench")
                return kzg.open_dev(v, L, point, t), t.state
            for _ in range(2):
                step()
            w = []
            for _ in range(7):
                a = time.perf_counter()
                step()
                w.append((time.perf_counter() - a) * 1e3)
            return statistics.median(w)
        res[f"world_{world}_rank0_median_ms"] = run_ranks(world, fn)[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("presum", "ipa", "open"))
    ap.add_argument("--merge", nargs="*")
    ap.add_argument("--log", type=int, default=None)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--outer", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.merge:
        res = {}
        for f in args.merge:
            with open(f) as fh:
                res[os.path.splitext(os.path.basename(f))[0]] = json.load(fh)
    else:
        if args.log is None:
            args.log = 22 if args.part == "presum" else 20
        res = {"presum": part_presum, "ipa": part_ipa, "open": part_open}[args.part](args)
    txt = json.dumps(res, indent=1, sort_keys=True)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
