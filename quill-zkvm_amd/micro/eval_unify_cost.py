"""The regions that run the polynomial-evaluation kernel, for comparing two
builds of the library (QG_LIB names the build; unset: the in-tree one):
  * kzg_open_check of one ML opening (open_dev) at 2^n evaluations;
  * fold_eval of the folded ML opening at 2^n;
  * fold_eval and kzg_open_check of the folded inner-product argument at each
    of --ipa-logs, with QG_EVAL_PAIRED 0 and 1.
One process measures one build: every figure is the median of --inner calls
with event timing on, the cases taken in turn.  micro/eval_lib_ab.sh alternates
the builds, one process each, and --summarize joins the processes' files: per
region and build the list of medians, its range, and whether the result's
median of medians lies within or below the parent's range or above it by no
more than the parent's spread.

  QG_LIB=<libquill_gpu.so> python quill-zkvm_amd/micro/eval_unify_cost.py
      [--log 22] [--ipa-logs 20,22] [--inner 7] --out <file>
  python quill-zkvm_amd/micro/eval_unify_cost.py --summarize <dir> --out <file>
      (files <dir>/<build>_<round>.json; the build named "parent" is the yardstick)"""
import argparse
import contextlib
import glob
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "quill-zkvm_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
if os.environ.get("QG_LIB"):  # A/B builds of the library (micro benchmark only)
    import quill_amd._lib as _L
    _L.LIB_PATH = os.path.abspath(os.environ["QG_LIB"])

TAU = 0x5155494C4C5F54415521
REGIONS = ("fold_eval", "kzg_open_check")


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


def measure(args):
    import quill_amd as q
    from quill_oracle import R_MOD as R
    dev = q.Device(0)
    N = 1 << args.log
    pcs = q.KZG.trusted_setup(N, TAU, dev)
    rnd = random.Random(args.log)
    point = [rnd.randrange(R) for _ in range(args.log)]
    vec = q.DeviceVec(dev, N).fill_random(0xF01D)
    g = q.DeviceVec(dev, N).fill_random(0xF01E)
    folding = pcs.folding()
    cases = {"mle_open_2^%d" % args.log:
             (lambda: pcs.open_dev(vec, N, point, q.Transcript(b"eval_unify")), None),
             "mle_open_folded_2^%d" % args.log:
             (lambda: folding.open_dev(vec, N, point, q.Transcript(b"eval_unify")), None)}
    for k in [int(x) for x in args.ipa_logs.split(",")]:
        f_k, g_k = vec.view(0, 1 << k), g.view(0, 1 << k)
        for paired in ("0", "1"):
            cases["ipa_folded_2^%d_paired%s" % (k, paired)] = (
                lambda f=f_k, g=g_k: q.FoldedInnerProductProof.prove(
                    f, g, pcs, q.Transcript(b"eval_unify")), paired)
    vals = {n: {r: [] for r in REGIONS} for n in cases}
    launches = {}
    for warm in (True, False):
        for _ in range(1 if warm else args.inner):
            for n, (fn, paired) in cases.items():
                with env("QG_EVAL_PAIRED", paired):
                    dev.enable_timing(True)
                    fn()
                    for r in REGIONS:
                        ms, cnt = dev.kernel_time(r)
                        if not warm:
                            vals[n][r].append(ms)
                        launches[n + "/" + r] = cnt
                    dev.enable_timing(False)
    out = {"library": os.environ.get("QG_LIB", "in-tree"), "inner": args.inner,
           "open_check_failures": dev.counter("open_check_failures"), "regions_recorded": launches,
           "median_ms": {n + "/" + r: statistics.median(v[r]) for n, v in vals.items()
                         for r in REGIONS if any(v[r])}}
    dev.close()
    return out


def summarize(d):
    runs = {}
    for path in sorted(glob.glob(os.path.join(d, "*_*.json"))):
        build = os.path.basename(path).rsplit("_", 1)[0]
        with open(path) as fh:
            runs.setdefault(build, []).append(json.load(fh))
    out = {"runs": runs, "regions": {}}
    base = runs["parent"]
    for key in base[0]["median_ms"]:
        row = {}
        for build, rs in runs.items():
            m = [r["median_ms"][key] for r in rs]
            row[build] = {"medians": m, "median": statistics.median(m), "min": min(m),
                          "max": max(m), "spread": max(m) - min(m)}
        p = row["parent"]
        for build in runs:
            if build != "parent":
                excess = row[build]["median"] - p["max"]
                row[build]["excess_over_parent_range_ms"] = max(0.0, excess)
                row[build]["within_margin"] = excess <= p["spread"]
        out["regions"][key] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=22)
    ap.add_argument("--ipa-logs", default="20,22")
    ap.add_argument("--inner", type=int, default=7)
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    out = summarize(args.summarize) if args.summarize else measure(args)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(json.dumps(out.get("regions", out.get("median_ms")), sort_keys=True))


if __name__ == "__main__":
    main()
