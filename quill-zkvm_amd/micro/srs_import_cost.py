"""Cost of bringing an SRS of 2^k points onto one device:
  * qg_srs_upload of trusted Montgomery limbs (the unvalidated baseline),
    qg_srs_import of the same points as uncompressed and as compressed
    ark-serialize bytes (decoded and validated on the device), wall time;
  * k_g1_decode's own time (region g1_decode) beside the table build
    (region srs_shift: k_srs_pack and the W - 1 k_srs_shift passes);
  * qg_srs_check_powers beside two lone qg_msm_g1_dev calls of the same length.
Every figure is a median of --inner calls, repeated --outer times, the cases
interleaved call by call; `spread` is max - min of the repeated medians.

  python quill-zkvm_amd/micro/srs_import_cost.py [--logs 20,24] [--inner 3] [--outer 3]
      [--out profiles/srs_import.json]
Prints one JSON object; --out also writes it (after every size)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "quill-zkvm_amd"))

TAU = 0x5155494C4C5F535253


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
    import numpy as np
    from quill_amd import Srs
    n = 1 << k
    gen = Srs.generate(dev, TAU, n)
    xy, inf = gen.download_raw()
    unc = np.frombuffer(gen.to_bytes(compressed=False), dtype=np.uint8)
    cmp_ = np.frombuffer(gen.to_bytes(compressed=True), dtype=np.uint8)
    g2 = q.g2_generator()
    g2pts = [g2, q.g2_mul(g2, TAU)]
    g1 = (1, 2)
    assert gen.check_powers(g1, g2pts)

    def upload():
        Srs.upload_raw(dev, xy, inf).close()

    def imp(data, compressed):
        def step():
            Srs.from_bytes(dev, data, compressed).close()
        return step

    cases = {"upload": upload, "import_uncompressed": imp(unc, False),
             "import_compressed": imp(cmp_, True)}
    for step in cases.values():
        step()
    res = {"points": n, "window_bits_tables": list(gen.window_info()),
           "wall_ms": interleaved(cases, inner, outer, wall_ms)}

    # the decode kernel beside the table build, timing on (enabling resets the regions)
    imports = ("import_uncompressed", "import_compressed")
    regions = ("g1_decode", "srs_shift")
    meds = {r: {name: [] for name in imports} for r in regions}
    for _ in range(outer):
        vals = {r: {name: [] for name in imports} for r in regions}
        for _ in range(inner):
            for name in imports:
                dev.enable_timing(True)
                cases[name]()
                for r in regions:
                    vals[r][name].append(dev.kernel_time(r)[0])
        for r in regions:
            for name in imports:
                meds[r][name].append(statistics.median(vals[r][name]))
    dev.enable_timing(False)
    for r in regions:
        res[r + "_ms"] = {name: summary(m) for name, m in meds[r].items()}

    # the powers check beside two lone MSMs of the same length
    v = q.DeviceVec(dev, n).fill_random(0x535253 + k)

    def two_msms():
        gen.msm_dev(v, n)
        gen.msm_dev(v, n)

    def powers():
        assert gen.check_powers(g1, g2pts)

    chk = {"check_powers": powers, "two_msm_g1_dev": two_msms}
    for step in chk.values():
        step()
    res["check_ms"] = interleaved(chk, inner, outer, wall_ms)
    v.close()
    gen.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="20,24")
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--outer", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import quill_amd as q
    dev = q.Device(0)
    out = {"inner": args.inner, "outer": args.outer}
    for k in (int(s) for s in args.logs.split(",")):
        out[f"2^{k}"] = one_size(q, dev, k, args.inner, args.outer)
        txt = json.dumps(out, indent=1, sort_keys=True)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(txt + "\n")
    dev.close()
    print(txt)


if __name__ == "__main__":
    main()
