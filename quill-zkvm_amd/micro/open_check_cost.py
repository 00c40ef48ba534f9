"""Cost of the KZG quotient check (the kzg_open_check region) on one device:
its share of the additive device-busy split (qg_ctx_phase_split) of
  * one open_dev at 2^k evaluations (bench.py's mle_open shape), and
  * one HyperPlonk proof at 2^r rows (bench.py's hyperplonk shape),
and the wall time of both with QG_OPEN_CHECK=0 and =1 (A/B, interleaved).

  python quill-zkvm_amd/micro/open_check_cost.py [--log-mle 22] [--log-hp-rows 20]
      [--reps 5] [--out profiles/open_check_cost.json]
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
MLE_PHASES = ("eq_table", "inner_product", "s_polynomial", "kzg_division", "kzg_open_check",
              "msm_bucketing", "msm_bucketing_side", "msm_accumulate", "msm_reduce")
HP_PHASES = MLE_PHASES + ("sumcheck_round", "sumcheck_tail", "logup_column")


def ab(step, reps):
    """median wall ms of step() with the check off and on, interleaved"""
    ms = {"0": [], "1": []}
    for _ in range(reps):
        for mode in ("0", "1"):
            os.environ["QG_OPEN_CHECK"] = mode
            t0 = time.perf_counter()
            step()
            ms[mode].append((time.perf_counter() - t0) * 1e3)
    os.environ.pop("QG_OPEN_CHECK")
    return {"check_off_ms": statistics.median(ms["0"]), "check_on_ms": statistics.median(ms["1"]),
            "reps": reps}


def split(dev, step, phases):
    dev.enable_timing(True)
    step()
    parts = dev.phase_split(phases)
    dev.enable_timing(False)
    tot = sum(parts.values())
    return {"parts_ms": parts, "parts_sum_ms": tot, "kzg_open_check_ms": parts["kzg_open_check"],
            "kzg_open_check_share": parts["kzg_open_check"] / tot if tot else 0.0}


def mle(q, dev, k, reps):
    from quill_amd import KZG, Transcript
    n = 1 << k
    kzg = KZG(dev, q.Srs.generate(dev, TAU, n), n - 1)
    poly = q.DeviceVec(dev, n).fill_random(0x5155494C4C + 4)
    t = Transcript(b"MLPCS bench")
    point = [t.draw_field_element() for _ in range(k)]

    def step():
        return kzg.open_dev(poly, n, point, Transcript(b"MLPCS bench"))
    for _ in range(2):
        step()
    res = {"shape": f"open_dev at 2^{k} evaluations", **ab(step, reps), **split(dev, step, MLE_PHASES)}
    poly.close()
    kzg.srs.close()
    return res


def hyperplonk(q, dev, k, reps):
    from quill_amd import KZG, HyperPlonk, TraceWitness
    from quill_amd import examples as ex
    rows = 1 << k
    cws = [ex.fibonacci_circuit_and_trace(rows), ex.modified_fibonacci_circuit_and_trace(rows)]
    pcs = KZG.trusted_setup(max(c.num_cols() * c.num_rows() for c, _ in cws), TAU, dev)
    hp = HyperPlonk.preprocess([c for c, _ in cws], pcs)
    wits = []
    for c, w in cws:
        buf = q.DeviceVec(dev, rows * c.num_cols())
        for i, col in enumerate(w):
            q.DeviceVec.from_canonical(dev, col, out=buf, offset=i * rows)
        wits.append(TraceWitness.from_full(buf, c.num_cols()))

    def step():
        return hp.prove(pcs, wits)
    step()
    c0 = dev.counter("open_checks")
    step()
    res = {"shape": f"HyperPlonk prove at 2^{k} rows", "quotients_checked_per_proof":
           dev.counter("open_checks") - c0, **ab(step, reps), **split(dev, step, HP_PHASES)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-mle", type=int, default=22)
    ap.add_argument("--log-hp-rows", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import quill_amd as q
    dev = q.Device(0)
    out = {"mle_open": mle(q, dev, args.log_mle, args.reps)}
    if args.log_hp_rows > 0:
        out["hyperplonk"] = hyperplonk(q, dev, args.log_hp_rows, max(2, args.reps // 2))
    out["open_check_failures"] = dev.counter("open_check_failures")
    dev.close()
    txt = json.dumps(out, indent=1, sort_keys=True)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
