"""Cost of the folded ML opening (KZG.folding()), measured:
  * one ML opening at 2^n evaluations, plain against folded with
    QG_FOLD_FUSED=1 (the fused scan) and =0 (the unfused composition): wall ms, the additive device-busy split, and
    the kzg_division / fold_eval / lincomb regions of each;
  * HyperPlonk prove of the two config-5 circuits at 2^k rows in four variants
    (default, folding(), multi_open=True, both): wall ms, split, proof bytes;
    verification of a 2^v-row proof, sequential and batched, for the same four;
  * the roofline of the fused scan at the 2^n shape: its algorithmic HBM bytes
    at the copy bandwidth measured here (qg_buf_copy, read + write) against its
    products at the qg_microbench_fq_mul rate.
The cases alternate in one process; every figure is a median of --inner runs,
repeated --repeats times (the list of medians is kept, the median of them is
quoted).

  python quill-zkvm_amd/micro/fold_open_cost.py [--open-log 22] [--rows-log 20]
      [--verify-rows-log 14] [--inner 5] [--repeats 5] [--out profiles/fold_open.json]
Prints one JSON object; --out also writes it (after every section, so a run
that is cut short leaves what it measured).  (The committed
profiles/fold_open.json also carries `unchanged_defaults`: bench.py runs, parent
commit against this change, added to the file from their result lines.)"""
import argparse
import contextlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "quill-zkvm_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

TAU = 0x5155494C4C5F54415521
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
PHASES = ("msm_bucketing", "msm_bucketing_side", "msm_accumulate", "msm_reduce",
          "sumcheck_round", "sumcheck_tail", "logup_column", "eq_table", "inner_product",
          "s_polynomial", "kzg_division", "kzg_open_check", "fold_eval", "eq_multi",
          "mle_eval_multi", "lincomb")
REGIONS = ("kzg_division", "fold_eval", "lincomb", "kzg_open_check")


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def alternating(cases, inner, repeats):
    """{name: step() -> figure or dict of figures}: per repeat, `inner` rounds
    over the cases in turn; -> {name: {key: {"medians": [...], "median": m}}}"""
    meds = {n: {} for n in cases}
    for _ in range(repeats):
        vals = {n: {} for n in cases}
        for _ in range(inner):
            for n, step in cases.items():
                v = step()
                for k, x in (v.items() if isinstance(v, dict) else [("ms", v)]):
                    vals[n].setdefault(k, []).append(x)
        for n in cases:
            for k, xs in vals[n].items():
                meds[n].setdefault(k, []).append(statistics.median(xs))
    return {n: {k: {"medians": m, "median": statistics.median(m), "spread": max(m) - min(m),
                    "inner": inner, "repeats": repeats} for k, m in meds[n].items()}
            for n in cases}


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def open_case(q, dev, log_n, inner, repeats):
    N = 1 << log_n
    rnd = random.Random(log_n)
    pcs = q.KZG.trusted_setup(N, TAU, dev)
    vec = q.DeviceVec(dev, N).fill_random(0xF01D)
    point = [rnd.randrange(R) for _ in range(log_n)]
    variants = {"plain": (pcs, None), "folded_fused": (pcs.folding(), "1"),
                "folded_unfused": (pcs.folding(), "0")}

    def opener(key):
        view, fused = variants[key]

        def fn():
            with env("QG_FOLD_FUSED", fused):
                view.open_dev(vec, N, point, q.Transcript(b"fold_open_cost"))
        return fn

    def step(key):
        fn = opener(key)

        def run():
            # the wall time without event recording, then the regions of one more call
            out = {"wall_ms": wall_ms(fn)}
            dev.enable_timing(True)
            fn()
            for name in REGIONS:
                out[name + "_ms"] = dev.kernel_time(name)[0]
            dev.enable_timing(False)
            return out
        return run

    for key in variants:
        opener(key)()  # warm: scratch, pools, MSM tables
    res = alternating({k: step(k) for k in variants}, inner, repeats)
    for key in variants:
        dev.enable_timing(True)
        opener(key)()
        parts = dev.phase_split(PHASES)
        res[key]["msm_launches"] = dev.kernel_time("msm_accumulate")[1]
        dev.enable_timing(False)
        res[key]["phase_split_ms"] = parts
        res[key]["phase_split_sum_ms"] = sum(parts.values())
    fused, unfused = res["folded_fused"], res["folded_unfused"]
    a = fused["kzg_division_ms"]
    b_div, b_lin = unfused["kzg_division_ms"], unfused["lincomb_ms"]
    # the unfused kzg_division region contains its lincomb launch (nested regions)
    res["fused_scan_ms"] = a["median"]
    res["unfused_composition_ms"] = b_div["median"]
    res["unfused_lincomb_part_ms"] = b_lin["median"]
    res["plain_four_jobs_ms"] = res["plain"]["kzg_division_ms"]["median"]
    spread = max(a["spread"], b_div["spread"])
    res["spread_of_medians_ms"] = spread
    res["fused_is_default_ok"] = a["median"] <= b_div["median"] + spread
    # roofline of the fused scan: local pass reads both sources, apply pass reads
    # both again and writes two suffix vectors; per entry 1 product for the fold
    # and 2 for the two Horner chains, in each pass
    half = vec.view(0, N // 2)
    copy_ms = statistics.median([wall_ms(lambda: vec.copy_from(half, N // 2, 0))
                                 for _ in range(2 * inner + 1)])
    copy_gbs = 2 * 32 * (N // 2) / (copy_ms * 1e-3) / 1e9
    fq = dev.microbench_fq_mul()
    nbytes, products = 32 * N * (2 + 2 + 2), 2 * 3 * N
    hbm_ms, mul_ms = nbytes / (copy_gbs * 1e9) * 1e3, products / fq * 1e3
    res["roofline"] = {"algorithmic_bytes": nbytes, "products": products,
                       "copy_GBps_read_plus_write": copy_gbs, "fq_mul_per_s": fq,
                       "hbm_bound_ms": hbm_ms, "mul_bound_ms": mul_ms,
                       "bound_by": "hbm" if hbm_ms > mul_ms else "products",
                       "ms_over_larger_bound": a["median"] / max(hbm_ms, mul_ms),
                       "note": "the recursion's upper levels (1/32 of the entries) are in "
                               "the measured region and not in the model"}
    res["log_n"] = log_n
    vec.close()
    pcs.close()
    return res


def hyperplonk_setup(q, dev, rows_log):
    from quill_amd import KZG, HyperPlonk, TraceWitness
    from quill_amd import examples as ex
    rows = 1 << rows_log
    cws = [ex.fibonacci_circuit_and_trace(rows), ex.modified_fibonacci_circuit_and_trace(rows)]
    pcs = KZG.trusted_setup(max(c.num_cols() * c.num_rows() for c, _ in cws), TAU, dev)
    hp = HyperPlonk.preprocess([c for c, _ in cws], pcs)
    wits = []
    for c, w in cws:  # resident in HBM before the timed region, like bench.py
        buf = q.DeviceVec(dev, rows * c.num_cols())
        for i, col in enumerate(w):
            q.DeviceVec.from_canonical(dev, col, out=buf, offset=i * rows)
        wits.append(TraceWitness.from_full(buf, c.num_cols()))
    return pcs, hp, wits


VARIANTS = {"default": (False, False), "folding": (True, False),
            "multi_open": (False, True), "folding_multi_open": (True, True)}


def prove_case(q, dev, rows_log, inner, repeats):
    pcs, hp, wits = hyperplonk_setup(q, dev, rows_log)
    proofs = {}

    def run(name):
        fold, multi = VARIANTS[name]

        def fn():
            proofs[name] = hp.prove(pcs.folding() if fold else pcs, wits, multi_open=multi)
        return fn

    for name in VARIANTS:
        run(name)()
    res = alternating({n: (lambda n=n: wall_ms(run(n))) for n in VARIANTS}, inner, repeats)
    vk = hp.to_vk()
    for name in VARIANTS:
        dev.enable_timing(True)
        ms = wall_ms(run(name))
        parts = dev.phase_split(PHASES)
        res[name]["msm_launches"] = dev.kernel_time("msm_accumulate")[1]
        dev.enable_timing(False)
        res[name]["ms_with_phase_timing"] = ms
        res[name]["phase_split_ms"] = parts
        res[name]["phase_split_sum_ms"] = sum(parts.values())
        res[name]["proof_bytes"] = len(q.serialize(proofs[name]))
        proofs[name].verify(vk, pcs, batch=True, dev=dev)
    res["rows"] = 1 << rows_log
    pcs.close()
    return res


def verify_case(q, dev, rows_log, inner, repeats):
    pcs, hp, wits = hyperplonk_setup(q, dev, rows_log)
    vk = hp.to_vk()
    cases = {}
    for name, (fold, multi) in VARIANTS.items():
        proof = hp.prove(pcs.folding() if fold else pcs, wits, multi_open=multi)
        final = hp.last_transcript.state

        def run(kw, proof=proof, final=final):
            def fn():
                assert proof.verify(vk, pcs, **kw).state == final
            return lambda: wall_ms(fn)
        cases[name + "_sequential"] = run({})
        cases[name + "_batch"] = run({"batch": True})
    for step in cases.values():
        step()
    res = alternating(cases, inner, repeats)
    res["rows"] = 1 << rows_log
    pcs.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--open-log", type=int, default=22)
    ap.add_argument("--rows-log", type=int, default=20)
    ap.add_argument("--verify-rows-log", type=int, default=14)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sections", default="mle_open,verify,hyperplonk_prove")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import quill_amd as q
    dev = q.Device(0)
    out = {}
    sections = {"mle_open": lambda: open_case(q, dev, args.open_log, args.inner, args.repeats),
                "verify": lambda: verify_case(q, dev, args.verify_rows_log, args.inner,
                                              args.repeats),
                "hyperplonk_prove": lambda: prove_case(q, dev, args.rows_log, args.inner,
                                                       args.repeats)}
    for name in args.sections.split(","):
        out[name] = sections[name]()
        print("section done:", name, flush=True)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    dev.close()
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
