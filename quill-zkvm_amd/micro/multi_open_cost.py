"""Cost of the multi-point batch opening (quill_amd/multiopen.py), measured:
  * HyperPlonk prove of the two config-5 circuits at 2^k rows with
    multi_open=False against True: wall ms around the call (the prover ends on
    a synchronised stream) and the additive phase split of one more proof each;
  * the three streaming kernels at nvars variables with k points and P vectors:
    device ms from the library's HIP-event regions, against their algorithmic
    HBM bytes at the copy bandwidth measured here (qg_buf_copy, read + write)
    and against their product count at the qg_microbench_fq_mul rate;
  * verification of one 2^v-row proof in both modes, sequential and batch=True.
The cases alternate in one process; every figure is a median of --inner runs,
repeated --repeats times (the list of medians is kept, the median of them is
quoted).

  python quill-zkvm_amd/micro/multi_open_cost.py [--rows-log 20] [--nvars 23] [--k 11] [--P 3]
      [--verify-rows-log 14] [--inner 5] [--repeats 5] [--out profiles/multi_open.json]
Prints one JSON object; --out also writes it.  (The committed
profiles/multi_open.json also carries `unchanged_defaults`: ten bench.py runs,
parent commit against this change, added to the file from their result lines.)"""
import argparse
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
HP_PHASES = ("msm_bucketing", "msm_bucketing_side", "msm_accumulate", "msm_reduce",
             "sumcheck_round", "sumcheck_tail", "logup_column", "eq_table", "inner_product",
             "s_polynomial", "kzg_division", "eq_multi", "mle_eval_multi", "lincomb")


def alternating(cases, inner, repeats):
    """{name: step() -> figure}: per repeat, `inner` rounds over the cases in
    turn; -> {name: {"medians": [...], "median": m}}"""
    meds = {n: [] for n in cases}
    for _ in range(repeats):
        vals = {n: [] for n in cases}
        for _ in range(inner):
            for n, step in cases.items():
                vals[n].append(step())
        for n in cases:
            meds[n].append(statistics.median(vals[n]))
    return {n: {"medians": m, "median": statistics.median(m), "inner": inner,
                "repeats": repeats} for n, m in meds.items()}


def wall_ms(fn):
    def step():
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    return step


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


def prove_case(q, dev, rows_log, inner, repeats):
    pcs, hp, wits = hyperplonk_setup(q, dev, rows_log)
    proofs = {}

    def run(mode):
        def fn():
            proofs[mode] = hp.prove(pcs, wits, multi_open=mode)
        return fn

    for mode in (False, True):
        run(mode)()  # warm: scratch, pools, MSM tables
    res = alternating({"multi_open_false": wall_ms(run(False)),
                       "multi_open_true": wall_ms(run(True))}, inner, repeats)
    for mode, name in ((False, "multi_open_false"), (True, "multi_open_true")):
        dev.enable_timing(True)
        ms = wall_ms(run(mode))()
        parts = dev.phase_split(HP_PHASES)
        dev.enable_timing(False)
        res[name]["ms_with_phase_timing"] = ms
        res[name]["phase_split_ms"] = parts
        res[name]["phase_split_sum_ms"] = sum(parts.values())
        p = proofs[mode]
        res[name]["ml_openings"] = sum(
            2 + (len(tp.multi_openings) if tp.multi_openings is not None
                 else len(tp.openings_zero_check) + len(tp.openings_public) + 3)
            for tp in p.trace_proofs)
        res[name]["proof_bytes"] = len(q.serialize(p))
    vk = hp.to_vk()
    for mode in (False, True):
        proofs[mode].verify(vk, pcs, batch=True, dev=dev)
    a, b = res["multi_open_false"]["median"], res["multi_open_true"]["median"]
    res["rows"] = 1 << rows_log
    res["true_over_false"] = b / a
    res["multi_open_is_faster"] = b < a
    pcs.close()
    return res


def kernel_case(q, dev, nvars, k, P, inner, repeats):
    N = 1 << nvars
    rnd = random.Random(nvars)
    pts = [[rnd.randrange(R) for _ in range(nvars)] for _ in range(k)]
    ws = [rnd.randrange(R) for _ in range(k)]
    cs = [rnd.randrange(R) for _ in range(P)]
    vecs = [q.DeviceVec(dev, N).fill_random(10 + j) for j in range(P)]
    out = q.DeviceVec(dev, N)

    def timed(name, fn):
        def step():
            dev.enable_timing(True)
            fn()
            ms = dev.kernel_time(name)[0]
            dev.enable_timing(False)
            return ms
        return step

    def copy():
        out.copy_from(vecs[0])

    cases = {"eq_multi": timed("eq_multi", lambda: dev.eq_multi_dev(pts, ws, out=out)),
             "mle_eval_multi": timed("mle_eval_multi", lambda: dev.mle_eval_multi(vecs[0], pts)),
             "lincomb": timed("lincomb", lambda: dev.lincomb_dev(vecs, cs, N, out=out)),
             "copy_wall": wall_ms(copy)}
    for step in cases.values():
        step()
    res = alternating(cases, inner, repeats)
    fq = dev.microbench_fq_mul()
    copy_gbs = 2 * 32 * N / (res["copy_wall"]["median"] * 1e-3) / 1e9
    small = 32 * k * ((1 << (nvars // 2)) + (1 << (nvars - nvars // 2)))
    model = {"eq_multi": (32 * N + small, k * N),
             "mle_eval_multi": (32 * N + small, (k + k / 4) * N),
             "lincomb": (32 * (P + 1) * N, P * N)}
    for name, (nbytes, products) in model.items():
        ms = res[name]["median"]
        hbm_ms = nbytes / (copy_gbs * 1e9) * 1e3
        mul_ms = products / fq * 1e3
        res[name].update({"algorithmic_bytes": nbytes, "products": products,
                          "achieved_GBps": nbytes / (ms * 1e-3) / 1e9,
                          "achieved_products_per_s": products / (ms * 1e-3),
                          "hbm_bound_ms": hbm_ms, "mul_bound_ms": mul_ms,
                          "bound_by": "hbm" if hbm_ms > mul_ms else "products",
                          "ms_over_larger_bound": ms / max(hbm_ms, mul_ms)})
    res.update({"nvars": nvars, "k": k, "P": P, "fq_mul_per_s": fq,
                "copy_GBps_read_plus_write": copy_gbs,
                "note": "device ms of the library's timed region (small tables included); "
                        "mle_eval_multi counts k products per entry plus k / 4 (one more per "
                        "4-row tile for the low factor)"})
    for v in vecs + [out]:
        v.close()
    return res


def verify_case(q, dev, rows_log, inner, repeats):
    pcs, hp, wits = hyperplonk_setup(q, dev, rows_log)
    vk = hp.to_vk()
    cases = {}
    for mode in (False, True):
        proof = hp.prove(pcs, wits, multi_open=mode)
        final = hp.last_transcript.state

        def run(kw, proof=proof, final=final):
            def fn():
                assert proof.verify(vk, pcs, **kw).state == final
            return wall_ms(fn)
        tag = "multi_open_true" if mode else "multi_open_false"
        cases[tag + "_sequential"] = run({})
        cases[tag + "_batch"] = run({"batch": True})
    for step in cases.values():
        step()
    res = alternating(cases, inner, repeats)
    res["rows"] = 1 << rows_log
    pcs.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log", type=int, default=20)
    ap.add_argument("--nvars", type=int, default=23)
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--P", type=int, default=3)
    ap.add_argument("--verify-rows-log", type=int, default=14)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import quill_amd as q
    dev = q.Device(0)
    out = {"kernels": kernel_case(q, dev, args.nvars, args.k, args.P, args.inner, args.repeats),
           "verify": verify_case(q, dev, args.verify_rows_log, args.inner, args.repeats),
           "hyperplonk_prove": prove_case(q, dev, args.rows_log, args.inner, args.repeats)}
    dev.close()
    txt = json.dumps(out, indent=1, sort_keys=True)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
