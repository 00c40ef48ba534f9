"""Cost of the lookup multiplicities (qg_lookup_multiplicities_dev) on one
device: device time by kernel group (lookup_build / lookup_count /
lookup_finish, HIP events) for 2 columns x 2^22 source rows against tables of
2^8 rows (every count on 256 addresses), 2^16 and 2^20 rows, and the
qg_logup_column_dev time on the same 2^22 rows as the yardstick, all in one
process with the cases interleaved.  Every figure is a median of --reps calls;
the whole measurement is repeated --medians times, and the spread of those
medians is what the 2^8 vs 2^20 comparison is judged against.

  python quill-zkvm_amd/micro/lookup_mult_cost.py [--log-src 22] [--reps 5]
      [--medians 5] [--out profiles/lookup_mult.json]
Prints one JSON object; --out also writes it."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "quill-zkvm_amd"))

HBM_BYTES_PER_S = 8e12  # the peak DESIGN.md prices every kernel against
GROUPS = ("lookup_build", "lookup_count", "lookup_finish")
TABLE_LOGS = (8, 16, 20)


def timed(dev, step, groups):
    dev.enable_timing(True)
    step()
    ms = {g: dev.kernel_time(g)[0] for g in groups}
    dev.enable_timing(False)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-src", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--medians", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import quill_amd as q
    from quill_amd import VirtualPolyExpr as E, VirtualPolynomialStore
    from quill_amd.logup import logup_column_device, lookup_multiplicities
    dev = q.Device(0)
    ns = 1 << args.log_src
    rnd = np.random.RandomState(22)
    cases = {}
    for lt in TABLE_LOGS:
        nt = 1 << lt
        j = np.arange(nt, dtype=np.uint64)
        idx = rnd.randint(0, nt, size=ns).astype(np.uint64)
        ss, ds = VirtualPolynomialStore(args.log_src, dev), VirtualPolynomialStore(lt, dev)
        for col in (idx, idx ^ np.uint64(42)):
            ss.allocate_polynomial(q.DeviceVec.from_u64(dev, col))
        for col in (j, j ^ np.uint64(42)):
            ds.allocate_polynomial(q.DeviceVec.from_u64(dev, col))
        sc = [ss.new_virtual_from_input(0), ss.new_virtual_from_input(1)]
        dc = [ds.new_virtual_from_input(0), ds.new_virtual_from_input(1)]

        def step(ss=ss, sc=sc, ds=ds, dc=dc):
            lookup_multiplicities(ss, sc, ds, dc).close()
        # the count is right before it is timed: every row found, m sums to the rows
        m = lookup_multiplicities(ss, sc, ds, dc)
        want = np.bincount(idx.astype(np.int64), minlength=nt)
        got = m.to_numpy()
        ref = q.DeviceVec.from_u64(dev, want.astype(np.uint64))
        assert np.array_equal(got, ref.to_numpy()), "multiplicities differ from the host count"
        m.close()
        ref.close()
        cases[lt] = (step, ss)
    # the yardstick: the log-derivative column over the same 2^22 source rows
    ss = cases[TABLE_LOGS[0]][1]
    out_col = q.DeviceVec(dev, ns)
    h = E.Input(0) + E.Const(0xA1FA) * E.Input(1)

    def logup_step():
        logup_column_device(dev, args.log_src, ss.polynomials, h, 0xBE7A, out_col)
    for step, _ in cases.values():
        step()
    logup_step()

    runs = []  # one dict of medians per repetition
    for _ in range(args.medians):
        samples = {lt: [] for lt in TABLE_LOGS}
        logup = []
        for _ in range(args.reps):  # interleaved: one call of every case per round
            for lt in TABLE_LOGS:
                samples[lt].append(timed(dev, cases[lt][0], GROUPS))
            logup.append(timed(dev, logup_step, ("logup_column",))["logup_column"])
        med = {"logup_column_ms": statistics.median(logup)}
        for lt in TABLE_LOGS:
            parts = {g: statistics.median(s[g] for s in samples[lt]) for g in GROUPS}
            parts["total_ms"] = statistics.median(sum(s.values()) for s in samples[lt])
            med[f"table_2p{lt}"] = parts
        runs.append(med)

    def over_runs(f):
        v = [f(r) for r in runs]
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}
    res = {"source_rows": ns, "columns": 2, "reps_per_median": args.reps,
           "medians": args.medians, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S,
           "logup_column_ms": over_runs(lambda r: r["logup_column_ms"])}
    for lt in TABLE_LOGS:
        nt = 1 << lt
        # algorithmic bytes: every input word read once, every output word written once
        alg = 2 * 32 * (ns + nt) + 32 * nt
        tot = over_runs(lambda r: r[f"table_2p{lt}"]["total_ms"])
        res[f"table_2p{lt}"] = {
            "table_rows": nt, "algorithmic_bytes": alg, "total_ms": tot,
            **{g: over_runs(lambda r, g=g: r[f"table_2p{lt}"][g]) for g in GROUPS},
            "fraction_of_hbm": alg / (tot["median"] * 1e-3) / HBM_BYTES_PER_S,
            "over_logup_column": tot["median"] / res["logup_column_ms"]["median"]}
    small, large = res["table_2p8"]["total_ms"], res["table_2p20"]["total_ms"]
    spread = max(small["max"] - small["min"], large["max"] - large["min"])
    res["contention_check"] = {
        "table_2p8_minus_2p20_ms": small["median"] - large["median"],
        "spread_of_medians_ms": spread,
        "holds": small["median"] - large["median"] <= spread}
    dev.close()
    txt = json.dumps(res, indent=1, sort_keys=True)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
