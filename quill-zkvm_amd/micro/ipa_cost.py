"""Cost of InnerProductProof::prove (qg_ipa_prove_dev) on one device, with
resident inputs, at 2^k coefficients per operand:
  * its wall time, and the same process's qg_mle_open_dev at the same size
    for scale (the IPA does one more forward NTT and three more MSMs);
  * the additive device-busy split (qg_ctx_phase_split) of one call;
  * the kzg_division region with QG_IPA_PAIRED=1 (three paired suffix-Horner
    jobs) against =0 (six single jobs).
Every figure is a median of --inner calls, repeated --outer times, the cases
interleaved call by call; `spread` is max - min of the repeated medians.

  python quill-zkvm_amd/micro/ipa_cost.py [--logs 20,22] [--inner 5] [--outer 5]
      [--out profiles/ipa_cost.json]
Prints one JSON object; --out also writes it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "quill-zkvm_amd"))

TAU = 0x5155494C4C5F54415521
PHASES = ("eq_table", "inner_product", "s_polynomial", "kzg_division", "kzg_open_check",
          "msm_bucketing", "msm_bucketing_side", "msm_accumulate", "msm_reduce")


def summary(medians):
    return {"medians": medians, "median": statistics.median(medians),
            "spread": max(medians) - min(medians)}


def interleaved(cases, inner, outer, measure):
    """{name: summary} of measure(name, step) over the cases, interleaved call by call"""
    meds = {name: [] for name in cases}
    for _ in range(outer):
        vals = {name: [] for name in cases}
        for _ in range(inner):
            for name, step in cases.items():
                vals[name].append(measure(name, step))
        for name in cases:
            meds[name].append(statistics.median(vals[name]))
    return {name: summary(m) for name, m in meds.items()}


def wall_ms(_name, step):
    t0 = time.perf_counter()
    step()
    return (time.perf_counter() - t0) * 1e3


def one_size(q, dev, k, inner, outer):
    from quill_amd import KZG, InnerProductProof, Transcript
    n = 1 << k
    kzg = KZG(dev, q.Srs.generate(dev, TAU, n), n - 1)
    f = q.DeviceVec(dev, n).fill_random(0x495041 + k)
    g = q.DeviceVec(dev, n).fill_random(0x495042 + k)
    t = Transcript(b"IPA bench")
    point = [t.draw_field_element() for _ in range(k)]

    def ipa(paired):
        def step():
            os.environ["QG_IPA_PAIRED"] = paired
            return InnerProductProof.prove(f, g, kzg, Transcript(b"IPA bench"))
        return step

    def mle():
        return kzg.open_dev(f, n, point, Transcript(b"MLPCS bench"))

    cases = {"ipa_paired": ipa("1"), "ipa_single": ipa("0"), "mle_open": mle}
    for step in cases.values():
        for _ in range(2):
            step()
    assert cases["ipa_paired"]() == cases["ipa_single"]()
    res = {"coefficients": n, "wall_ms": interleaved(cases, inner, outer, wall_ms)}

    # the regions of one call, timing on (the events add host time: the wall
    # figures above are taken with timing off); enabling resets the regions
    parts = {}

    def division_ms(name, step):
        dev.enable_timing(True)
        step()
        parts[name] = dev.phase_split(PHASES)
        return parts[name]["kzg_division"]

    ab = {name: cases[name] for name in ("ipa_paired", "ipa_single")}
    div = interleaved(ab, inner, outer, division_ms)
    division_ms("mle_open", mle)
    dev.enable_timing(False)
    os.environ.pop("QG_IPA_PAIRED", None)
    diff = div["ipa_single"]["median"] - div["ipa_paired"]["median"]
    noise = max(div["ipa_single"]["spread"], div["ipa_paired"]["spread"])
    res["kzg_division_ms"] = {**div, "single_minus_paired": diff, "noise": noise,
                              "faster": ("paired" if diff > 0 else "single") if abs(diff) > noise
                              else "within noise"}
    res["parts_ms"] = {name: {**p, "sum": sum(p.values())} for name, p in parts.items()}
    for v in (f, g):
        v.close()
    kzg.srs.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="20,22")
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--outer", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import quill_amd as q
    dev = q.Device(0)
    out = {"inner": args.inner, "outer": args.outer}
    for k in (int(s) for s in args.logs.split(",")):
        out[f"2^{k}"] = one_size(q, dev, k, args.inner, args.outer)
    out["open_check_failures"] = dev.counter("open_check_failures")
    dev.close()
    txt = json.dumps(out, indent=1, sort_keys=True)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
