"""Cost of the folded inner-product argument (FoldedInnerProductProof), measured:
  * one proof over two resident vectors of 2^n coefficients, qg_ipa_prove_dev
    (the yardstick, same build) against qg_ipa_prove_folded_dev with the six
    values from two single evaluation calls (QG_EVAL_PAIRED=0) and from the
    two-point kernel (=1), and with the fused scan (QG_FOLD_FUSED=1): wall ms,
    the kzg_division / fold_eval / lincomb / kzg_open_check regions, the
    additive device-busy split and the MSM count of each;
  * which fold_eval route and which scan is faster beyond the spread of the
    repeated medians;
  * the roofline of the two-point kernel at that shape: its algorithmic HBM
    bytes at the copy bandwidth measured here (qg_buf_copy, read + write)
    against its products at the qg_microbench_fq_mul rate;
  * verification of one proof, sequential and deferred, plain against folded,
    and the proof bytes.
The cases alternate in one process; every figure is a median of --inner runs,
repeated --repeats times (the list of medians is kept, the median of them is
quoted, with the spread max - min of the medians).

  python quill-zkvm_amd/micro/fold_ipa_cost.py [--logs 20,22] [--verify-log 12]
      [--inner 5] [--repeats 5] [--out profiles/fold_ipa.json]
Prints one JSON object; --out also writes it (after every section, so a run
that is cut short leaves what it measured).  (The committed
profiles/fold_ipa.json also carries `unchanged_defaults`: bench.py runs, parent
commit against this change, added to the file from their result lines.)"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "quill-zkvm_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

TAU = 0x5155494C4C5F54415521
PHASES = ("msm_bucketing", "msm_bucketing_side", "msm_accumulate", "msm_reduce",
          "inner_product", "s_polynomial", "kzg_division", "kzg_open_check", "fold_eval",
          "lincomb")
REGIONS = ("kzg_division", "fold_eval", "lincomb", "kzg_open_check", "s_polynomial")
DOMAIN = b"fold_ipa_cost"


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def alternating(cases, inner, repeats):
    """{name: step() -> dict of figures}: per repeat, `inner` rounds over the
    cases in turn; -> {name: {key: {"medians": [...], "median": m, "spread": s}}}"""
    meds = {n: {} for n in cases}
    for _ in range(repeats):
        vals = {n: {} for n in cases}
        for _ in range(inner):
            for n, step in cases.items():
                for k, x in step().items():
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


# name -> (folded, QG_EVAL_PAIRED, QG_FOLD_FUSED)
VARIANTS = {"plain": (False, None, None), "folded_single_eval": (True, "0", None),
            "folded_paired_eval": (True, "1", None), "folded_fused_scan": (True, "0", "1")}


def faster(a, b):
    """a is faster than b beyond the spread of the repeated medians"""
    return a["median"] + max(a["spread"], b["spread"]) < b["median"]


def prove_case(q, dev, log_n, inner, repeats):
    N = 1 << log_n
    pcs = q.KZG.trusted_setup(N, TAU, dev)
    f = q.DeviceVec(dev, N).fill_random(0x1FA0 + log_n)
    g = q.DeviceVec(dev, N).fill_random(0x1FB0 + log_n)
    proofs = {}

    def prover(key):
        folded, paired, fused = VARIANTS[key]
        cls = q.FoldedInnerProductProof if folded else q.InnerProductProof

        def fn():
            with env(QG_EVAL_PAIRED=paired, QG_FOLD_FUSED=fused):
                proofs[key] = cls.prove(f, g, pcs, q.Transcript(DOMAIN))
        return fn

    def step(key):
        fn = prover(key)

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

    for key in VARIANTS:
        prover(key)()  # warm: scratch, pools, MSM tables
    assert proofs["folded_single_eval"] == proofs["folded_paired_eval"] == proofs["folded_fused_scan"]
    res = alternating({k: step(k) for k in VARIANTS}, inner, repeats)
    for key in VARIANTS:
        dev.enable_timing(True)
        prover(key)()
        parts = dev.phase_split(PHASES)
        res[key]["msm_launches"] = dev.kernel_time("msm_accumulate")[1]
        dev.enable_timing(False)
        res[key]["phase_split_ms"] = parts
        res[key]["phase_split_sum_ms"] = sum(parts.values())
        res[key]["proof_bytes"] = len(q.serialize(proofs[key]))
    single, paired = res["folded_single_eval"], res["folded_paired_eval"]
    res["fold_eval"] = {"two_single_calls_ms": single["fold_eval_ms"],
                        "two_point_kernel_ms": paired["fold_eval_ms"],
                        "two_point_faster_beyond_spread": faster(paired["fold_eval_ms"],
                                                                 single["fold_eval_ms"]),
                        "single_faster_beyond_spread": faster(single["fold_eval_ms"],
                                                              paired["fold_eval_ms"])}
    comp, fused = single["kzg_division_ms"], res["folded_fused_scan"]["kzg_division_ms"]
    res["scan_P3"] = {"composition_ms": comp, "fused_ms": fused,
                      "composition_lincomb_part_ms": single["lincomb_ms"],
                      "fused_faster_beyond_spread": faster(fused, comp),
                      "composition_faster_beyond_spread": faster(comp, fused)}
    res["folded_faster_than_plain_beyond_spread"] = faster(single["wall_ms"],
                                                           res["plain"]["wall_ms"])
    # roofline of the evaluation at two points: the two-point kernel reads each of
    # the three vectors (f and g of N, S of N - 1 coefficients) once, the two
    # single calls read them twice; either way one product per coefficient and
    # point (the span stage and the shuffle tree add 1/32 of that and less)
    half = f.view(0, N // 2)
    copy_ms = statistics.median([wall_ms(lambda: f.copy_from(half, N // 2, 0))
                                 for _ in range(2 * inner + 1)])
    copy_gbs = 2 * 32 * (N // 2) / (copy_ms * 1e-3) / 1e9
    fq = dev.microbench_fq_mul()
    products = 2 * (3 * N - 1)
    mul_ms = products / fq * 1e3
    roof = {"products": products, "copy_GBps_read_plus_write": copy_gbs, "fq_mul_per_s": fq,
            "mul_bound_ms": mul_ms}
    for name, reads, ms in (("two_point_kernel", 1, paired["fold_eval_ms"]["median"]),
                            ("two_single_calls", 2, single["fold_eval_ms"]["median"])):
        nbytes = 32 * (3 * N - 1) * reads
        hbm_ms = nbytes / (copy_gbs * 1e9) * 1e3
        roof[name] = {"algorithmic_bytes": nbytes, "hbm_bound_ms": hbm_ms,
                      "bound_by": "hbm" if hbm_ms > mul_ms else "products",
                      "measured_region_ms": ms,
                      "ms_over_larger_bound": ms / max(hbm_ms, mul_ms)}
    roof["note"] = ("the fold_eval region also holds the 192-byte copy to pinned memory; "
                    "qg_microbench_fq_mul is the Fq 4x64-limb rate, the kernel multiplies "
                    "29-bit-limb Fr values")
    res["roofline"] = roof
    res["log_n"] = log_n
    f.close()
    g.close()
    pcs.close()
    return res


def verify_case(q, dev, log_n, inner, repeats):
    N = 1 << log_n
    pcs = q.KZG.trusted_setup(N, TAU, dev)
    f = q.DeviceVec(dev, N).fill_random(0x2FA0)
    g = q.DeviceVec(dev, N).fill_random(0x2FB0)
    c1, c2 = pcs.commit(f), pcs.commit(g)
    cases, out = {}, {}
    for name, cls in (("plain", q.InnerProductProof), ("folded", q.FoldedInnerProductProof)):
        t = q.Transcript(DOMAIN)
        proof = cls.prove(f, g, pcs, t)
        out[name + "_proof_bytes"] = len(q.serialize(proof))

        def sequential(proof=proof, final=t.state):
            tv = q.Transcript(DOMAIN)
            assert proof.verify(c1, c2, pcs, tv) and tv.state == final

        def deferred(proof=proof, final=t.state):
            view, tv = pcs.deferring(), q.Transcript(DOMAIN)
            assert proof.verify(c1, c2, view, tv) and tv.state == final
            view.check()
        cases[name + "_sequential"] = lambda fn=sequential: {"wall_ms": wall_ms(fn)}
        cases[name + "_deferred"] = lambda fn=deferred: {"wall_ms": wall_ms(fn)}
    for step in cases.values():
        step()
    out.update(alternating(cases, inner, repeats))
    out["log_n"] = log_n
    f.close()
    g.close()
    pcs.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="20,22")
    ap.add_argument("--verify-log", type=int, default=12)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import quill_amd as q
    dev = q.Device(0)
    out = {}

    def done(name):
        print("section done:", name, flush=True)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    for log_n in [int(x) for x in args.logs.split(",")]:
        out["prove_2^%d" % log_n] = prove_case(q, dev, log_n, args.inner, args.repeats)
        done("prove 2^%d" % log_n)
    out["verify"] = verify_case(q, dev, args.verify_log, args.inner, args.repeats)
    done("verify")
    dev.close()
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
