"""Costs around the sharded lookup multiplicities and the column materialiser,
device time by kernel group (HIP events), one part per run:

  --part single        micro/lookup_mult_cost.py's own measurement (its medians
                       and their spread) on the library QG_LIB names: run on the
                       parent's build and on this one, alternating, to see that
                       the single-context count did not move
  --part materialiser  k_expr_column ("expr_column") for a + 256 b over 2 columns
                       x 2^22 rows, next to the count of those rows against a
                       2^16-row table
  --part sharded       the per-rank split gather / build / count / exchange /
                       finish at world 2 and 4: ranks are host threads over the
                       loopback communicator SHARING ONE GPU, so the figures are
                       contended (the ranks' kernels interleave and a collective
                       waits for the slowest rank): not multi-GPU figures
  --part modes         the two sharded table modes (replicated / partitioned,
                       qg_lookup_multiplicities_dev_ex) at world 4 on two shapes:
                       "small_table" (2^16 global table rows under 2^log-src
                       source rows) and "table_is_source" (2^log-big distinct
                       rows per rank in both).  Per rank: device time by kernel
                       group, lookup_exchange_bytes per call and the lookup's
                       arena scratch.  Each rank drives one context per mode and
                       alternates the modes call by call in one process.  The
                       same caveat: the loopback ranks share one GPU and their
                       collectives are device copies, so the times describe work
                       done, not link time.  On a library without the _ex entry
                       (QG_LIB = the parent's build) only "replicated" is run;
                       --modes replicated runs it alone on this build too, which
                       is the like-for-like comparison of two builds.
  --merge a.json ...   one object from the parts' outputs (--out writes it)

  QG_LIB=<libquill_gpu.so> python quill-zkvm_amd/micro/lookup_sharded_cost.py
      --part <p> [--log-src 22] [--reps 5] [--medians 5] [--out f.json]"""
import argparse
import json
import os
import statistics
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
if os.environ.get("QG_LIB"):  # A/B builds of the library (micro benchmark only)
    import quill_amd._lib as _L
    _L.LIB_PATH = os.path.abspath(os.environ["QG_LIB"])
    import ctypes
    _old = ctypes.CDLL(_L.LIB_PATH)  # an older build lacks the newer entries: not bound
    for _k in [k for k in _L.PROTOTYPES if not hasattr(_old, k)]:
        del _L.PROTOTYPES[_k]

HBM_BYTES_PER_S = 8e12
SHARD_GROUPS = ("lookup_gather", "lookup_build", "lookup_count", "lookup_exchange",
                "lookup_finish")


def timed(dev, step, groups):
    dev.enable_timing(True)
    step()
    ms = {g: dev.kernel_time(g)[0] for g in groups}
    dev.enable_timing(False)
    return ms


def spread(vals):
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}


def part_single(args):
    import lookup_mult_cost
    sys.argv = [sys.argv[0], "--log-src", str(args.log_src), "--reps", str(args.reps),
                "--medians", str(args.medians)] + (["--out", args.out] if args.out else [])
    lookup_mult_cost.main()


def part_materialiser(args):
    import quill_amd as q
    from quill_amd import VirtualPolyExpr as E, VirtualPolynomialStore
    from quill_amd.logup import expr_column, lookup_multiplicities
    dev = q.Device(0)
    ns, lt = 1 << args.log_src, 16
    rnd = np.random.RandomState(7)
    a = rnd.randint(0, 256, size=ns).astype(np.uint64)
    b = rnd.randint(0, 256, size=ns).astype(np.uint64)
    j = np.arange(1 << lt, dtype=np.uint64)
    ss, ds = VirtualPolynomialStore(args.log_src, dev), VirtualPolynomialStore(lt, dev)
    for col in (a, b, b, a):
        ss.allocate_polynomial(q.DeviceVec.from_u64(dev, col))
    for col in ((j & np.uint64(255)) + np.uint64(256) * (j >> np.uint64(8)),
                (j >> np.uint64(8)) + np.uint64(256) * (j & np.uint64(255))):
        ds.allocate_polynomial(q.DeviceVec.from_u64(dev, col))
    pack = [ss.new_virtual_from_expr(E.Input(0) + E.Const(256) * E.Input(1)),
            ss.new_virtual_from_expr(E.Input(2) + E.Const(256) * E.Input(3))]
    dc = [ds.new_virtual_from_input(0), ds.new_virtual_from_input(1)]
    # right before it is timed: the packed columns against the host's
    got = expr_column(ss, pack[0])
    ref = q.DeviceVec.from_u64(dev, a + np.uint64(256) * b)
    assert got.first_mismatch(ref) == -1, "materialised column differs from the host's"
    ref.close()
    cols = [got, expr_column(ss, pack[1])]
    ms_ = VirtualPolynomialStore(args.log_src, dev)
    plain = [ms_.new_virtual_from_input(ms_.allocate_polynomial(c)) for c in cols]

    def mat():
        for p in pack:
            expr_column(ss, p).close()

    def count():
        lookup_multiplicities(ms_, plain, ds, dc).close()

    def both():
        lookup_multiplicities(ss, pack, ds, dc, materialise=True).close()
    for f in (mat, count, both):
        f()
    cg = ("lookup_build", "lookup_count", "lookup_finish")
    runs = []
    for _ in range(args.medians):
        m, c, t = [], [], []
        for _ in range(args.reps):
            m.append(timed(dev, mat, ("expr_column",))["expr_column"])
            c.append(sum(timed(dev, count, cg).values()))
            t.append(sum(timed(dev, both, cg + ("expr_column",)).values()))
        runs.append((statistics.median(m), statistics.median(c), statistics.median(t)))
    alg = 2 * 3 * 32 * ns  # per column: two words read, one written, per row
    mat_ms = spread([r[0] for r in runs])
    res = {"source_rows": ns, "columns": 2, "table_rows": 1 << lt, "expression": "a + 256 b",
           "reps_per_median": args.reps, "medians": args.medians,
           "expr_column_ms_two_columns": mat_ms,
           "count_ms": spread([r[1] for r in runs]),
           "materialise_and_count_ms": spread([r[2] for r in runs]),
           "algorithmic_bytes": alg,
           "fraction_of_hbm": alg / (mat_ms["median"] * 1e-3) / HBM_BYTES_PER_S}
    res["expr_column_over_count"] = mat_ms["median"] / res["count_ms"]["median"]
    dev.close()
    return res


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


def part_sharded(args):
    import quill_amd as q
    from quill_amd import VirtualPolynomialStore
    from quill_amd.logup import lookup_multiplicities
    ns, lt = 1 << args.log_src, 16
    nt = 1 << lt
    rnd = np.random.RandomState(16)
    idx = rnd.randint(0, nt, size=ns).astype(np.uint64)
    j = np.arange(nt, dtype=np.uint64)
    want = np.bincount(idx.astype(np.int64), minlength=nt).astype(np.uint64)
    res = {"source_rows_global": ns, "table_rows_global": nt, "columns": 2,
           "reps_per_median": args.reps, "medians": args.medians,
           "note": "loopback ranks are host threads sharing one GPU: contended figures, "
                   "not multi-GPU figures; gather and exchange include the wait for the "
                   "slowest rank"}
    for world in (2, 4):
        S, T = ns // world, nt // world

        def fn(dev, rank, world, S=S, T=T):
            ss = VirtualPolynomialStore(args.log_src, dev)
            ds = VirtualPolynomialStore(lt, dev)
            sl, tl = slice(rank * S, (rank + 1) * S), slice(rank * T, (rank + 1) * T)
            for col in (idx[sl], idx[sl] ^ np.uint64(42)):
                ss.allocate_polynomial(q.DeviceVec.from_u64(dev, col))
            for col in (j[tl], j[tl] ^ np.uint64(42)):
                ds.allocate_polynomial(q.DeviceVec.from_u64(dev, col))
            sc = [ss.new_virtual_from_input(0), ss.new_virtual_from_input(1)]
            dc = [ds.new_virtual_from_input(0), ds.new_virtual_from_input(1)]
            m = lookup_multiplicities(ss, sc, ds, dc)
            ref = q.DeviceVec.from_u64(dev, want[tl])
            assert m.first_mismatch(ref) == -1, "sharded multiplicities differ from the host count"
            m.close()
            ref.close()

            def step():
                lookup_multiplicities(ss, sc, ds, dc).close()
            runs = []
            for _ in range(args.medians):
                s = [timed(dev, step, SHARD_GROUPS) for _ in range(args.reps)]
                med = {g: statistics.median(x[g] for x in s) for g in SHARD_GROUPS}
                med["total_ms"] = statistics.median(sum(x.values()) for x in s)
                runs.append(med)
            return {k: spread([r[k] for r in runs]) for k in SHARD_GROUPS + ("total_ms",)}
        per_rank = run_ranks(world, fn)
        res[f"world_{world}"] = {"source_rows_per_rank": S, "table_rows_per_rank": T,
                                 "ranks": per_rank}
    return res


MODE_GROUPS = {"replicated": SHARD_GROUPS,
               "partitioned": ("lookup_dedup", "lookup_route", "lookup_exchange", "lookup_owner",
                               "lookup_finish")}


def part_modes(args):
    import ctypes as C
    import quill_amd as q
    from quill_amd._lib import check
    L = q.lib()
    has_ex = hasattr(L, "qg_lookup_multiplicities_dev_ex")
    modes = ("replicated", "partitioned") if has_ex else ("replicated",)
    if args.modes:
        modes = tuple(m for m in modes if m in args.modes.split(","))
    world = 4
    res = {"world": world, "columns": 2, "modes": list(modes), "reps_per_median": args.reps,
           "medians": args.medians,
           "note": "loopback ranks are host threads sharing one GPU and their collectives are "
                   "device copies: the times describe work done, not link time; exchange "
                   "groups include the wait for the slowest rank"}

    def count(dev, sc, dc, out, mode):
        miss = C.c_int64(-1)
        sp = (C.c_void_p * 2)(*[v.h.value for v in sc])
        tp = (C.c_void_p * 2)(*[v.h.value for v in dc])
        if has_ex:
            rc = L.qg_lookup_multiplicities_dev_ex(dev.h, 2, sp, sc[0].n, tp, dc[0].n, out.h,
                                                   C.byref(miss), 0 if mode == "replicated" else 1)
        else:
            rc = L.qg_lookup_multiplicities_dev(dev.h, 2, sp, sc[0].n, tp, dc[0].n, out.h,
                                                C.byref(miss))
        check(rc, dev.h)

    def counter(dev, name):
        v = C.c_uint64()
        check(L.qg_ctx_counter(dev.h, name.encode(), C.byref(v)), dev.h)
        return v.value

    shapes = {}
    ns, nt = 1 << args.log_src, 1 << 16
    rnd = np.random.RandomState(16)
    idx = rnd.randint(0, nt, size=ns).astype(np.uint64)
    shapes["small_table"] = (idx, np.arange(nt, dtype=np.uint64),
                             np.bincount(idx.astype(np.int64), minlength=nt).astype(np.uint64))
    nb = world << args.log_big
    shapes["table_is_source"] = (np.random.RandomState(20).permutation(nb).astype(np.uint64),
                                 np.arange(nb, dtype=np.uint64), np.ones(nb, dtype=np.uint64))
    for name, (src, tab, want) in shapes.items():
        S, T = len(src) // world, len(tab) // world
        groups = {m: q.Device.loopback_group(world) for m in modes}
        out, err = [None] * world, []

        def body(rank, src=src, tab=tab, want=want, S=S, T=T, groups=groups):
            try:
                sl, tl = slice(rank * S, (rank + 1) * S), slice(rank * T, (rank + 1) * T)
                ctx = {}
                for m in modes:
                    dev = q.Device(0)
                    dev.attach_loopback(groups[m], rank)
                    sc = [q.DeviceVec.from_u64(dev, c) for c in (src[sl], src[sl] ^ np.uint64(42))]
                    dc = [q.DeviceVec.from_u64(dev, c) for c in (tab[tl], tab[tl] ^ np.uint64(42))]
                    o_ = q.DeviceVec(dev, T)
                    count(dev, sc, dc, o_, m)  # warm, and checked right before it is timed
                    ref = q.DeviceVec.from_u64(dev, want[tl])
                    assert o_.first_mismatch(ref) == -1, "multiplicities differ from the host count"
                    ref.close()
                    ctx[m] = (dev, sc, dc, o_)
                runs = {m: [] for m in modes}
                bytes_per_call = {}
                for _ in range(args.medians):
                    samples = {m: [] for m in modes}
                    for _ in range(args.reps):
                        for m in modes:  # interleaved
                            dev, sc, dc, o_ = ctx[m]
                            b0 = (counter(dev, "lookup_exchange_bytes") if has_ex else 0)
                            samples[m].append(timed(dev, lambda: count(dev, sc, dc, o_, m),
                                                    MODE_GROUPS[m]))
                            if has_ex:
                                bytes_per_call[m] = counter(dev, "lookup_exchange_bytes") - b0
                    for m in modes:
                        med = {g: statistics.median(x[g] for x in samples[m])
                               for g in MODE_GROUPS[m]}
                        med["total_ms"] = statistics.median(sum(x.values()) for x in samples[m])
                        runs[m].append(med)
                r = {}
                for m in modes:
                    dev = ctx[m][0]
                    r[m] = {k: spread([x[k] for x in runs[m]])
                            for k in MODE_GROUPS[m] + ("total_ms",)}
                    if has_ex:
                        r[m]["lookup_exchange_bytes_per_call"] = bytes_per_call[m]
                        r[m]["lookup_scratch_bytes"] = counter(dev, "lookup_scratch_bytes")
                    for v in ctx[m][1] + ctx[m][2] + [ctx[m][3]]:
                        v.close()
                    dev.close()
                out[rank] = r
            except Exception as e:
                err.append(e)
        ths = [threading.Thread(target=body, args=(r,)) for r in range(world)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        for g in groups.values():
            q.lib().qg_loopback_destroy(g)
        if err:
            raise err[0]
        res[name] = {"source_rows_per_rank": S, "table_rows_per_rank": T, "ranks": out}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("single", "materialiser", "sharded", "modes"))
    ap.add_argument("--log-big", type=int, default=20)
    ap.add_argument("--modes", default=None,
                    help="part modes: comma list (replicated alone compares two builds)")
    ap.add_argument("--merge", nargs="*")
    ap.add_argument("--log-src", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--medians", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.part == "single":
        return part_single(args)
    if args.merge:
        res = {}
        for f in args.merge:
            with open(f) as fh:
                res[os.path.splitext(os.path.basename(f))[0]] = json.load(fh)
    else:
        res = {"materialiser": part_materialiser, "sharded": part_sharded,
               "modes": part_modes}[args.part](args)
    txt = json.dumps(res, indent=1, sort_keys=True)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
