"""Cost of verification, sequential against batched (qg_kzg_verify_batch):
  * one device-proved HyperPlonk proof of the two config-5 circuits at 2^k
    rows, verified by HyperPlonkProof.verify sequentially (one pairing check per
    KZG opening: the verifier as it was before batching, the yardstick), with
    batch=True and the host fold, and with batch=True and the device fold;
  * the fold alone (qg_kzg_batch_fold against qg_kzg_batch_fold_dev) and the
    whole accepting check (qg_kzg_verify_batch against _dev) on synthetic valid
    claim sets of n claims, and the smallest measured n from which the device
    fold is the faster one.
The synthetic claims are fabricated with the trapdoor: C = c g1 opened at x to
y has pi = ((c - y) / (tau - x)) g1, c and the quotient scalar walking
arithmetic progressions so that a point costs one group addition to make.
Every figure is a median of --inner calls (one call for a host fold of more
than 2^12 claims, which takes seconds).

  python quill-zkvm_amd/micro/verify_batch_cost.py [--rows-log 14] [--ns 4,16,64,1024,16384]
      [--inner 3] [--out profiles/verify_batch.json]
Prints one JSON object; --out also writes it."""
import argparse
import ctypes as C
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


def median_ms(step, inner):
    vals = []
    for _ in range(inner):
        t0 = time.perf_counter()
        step()
        vals.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals), "calls": inner}


def hyperplonk_case(q, dev, rows_log, inner):
    from quill_amd import KZG, HyperPlonk
    from quill_amd import examples as ex
    rows = 1 << rows_log
    cws = [ex.fibonacci_circuit_and_trace(rows), ex.modified_fibonacci_circuit_and_trace(rows)]
    pcs = KZG.trusted_setup(max(c.num_cols() * c.num_rows() for c, _ in cws), TAU, dev)
    hp = HyperPlonk.preprocess([c for c, _ in cws], pcs)
    proof = hp.prove(pcs, [w for _, w in cws])
    final = hp.last_transcript.state
    vk = hp.to_vk()
    view = pcs.deferring()
    from quill_amd.proof import _hyperplonk_verify
    _hyperplonk_verify(proof, vk, view)

    def run(**kw):
        def step():
            assert proof.verify(vk, pcs, **kw).state == final
        return step

    cases = {"sequential": run(), "batch_host_fold": run(batch=True),
             "batch_device_fold": run(batch=True, dev=dev)}
    for step in cases.values():
        step()  # warm: G2 subgroup memo, MSM scratch
    res = {name: median_ms(step, inner) for name, step in cases.items()}
    res["rows"] = rows
    res["traces"] = len(cws)
    res["pairing_checks_sequential"] = len(view.claims)
    res["pairing_checks_batched"] = 1
    res["deferred_replay_without_check"] = median_ms(
        lambda: _hyperplonk_verify(proof, vk, pcs.deferring()), inner)
    res["note"] = ("sequential = HyperPlonkProof.verify(vk, pcs), unchanged by batching: the "
                   "yardstick; wall ms on the host, device fold included where used")
    pcs.close()
    return res


def synthetic_claims(n, seed=0xBA7C4):
    import pairing_oracle as po
    R = po.R
    rnd = random.Random(seed)
    c0, dc, k0, dk = (rnd.randrange(1, R) for _ in range(4))
    Cp, Dc = po.g1_mul(po.G1_GEN, c0), po.g1_mul(po.G1_GEN, dc)
    Kp, Dk = po.g1_mul(po.G1_GEN, k0), po.g1_mul(po.G1_GEN, dk)
    out = []
    for i in range(n):
        c, k, x = (c0 + i * dc) % R, (k0 + i * dk) % R, rnd.randrange(R)
        out.append((Cp, x, (c - k * (TAU - x)) % R, Kp))
        Cp, Kp = po.g1_add(Cp, Dc), po.g1_add(Kp, Dk)
    return out


def fold_case(q, dev, vk, claims, n, inner):
    from quill_amd._lib import KzgClaim
    from quill_amd.pcs import _claim_c
    L = q.lib()
    arr = (KzgClaim * n)()
    for i, (Cm, x, y, pi) in enumerate(claims[:n]):
        arr[i] = _claim_c(Cm, q.KZGOpeningProof(x, y, pi))
    k = vk._vk()
    outs = {}

    def fold(on_dev):
        def step():
            lxy, rxy = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
            linf, rinf = C.c_uint8(), C.c_uint8()
            if on_dev:
                rc = L.qg_kzg_batch_fold_dev(dev.h, C.byref(k), arr, n, None, lxy, C.byref(linf),
                                             rxy, C.byref(rinf))
            else:
                rc = L.qg_kzg_batch_fold(C.byref(k), arr, n, None, lxy, C.byref(linf), rxy,
                                         C.byref(rinf))
            assert rc == 0, rc
            outs[on_dev] = (list(lxy), linf.value, list(rxy), rinf.value)
        return step

    def verify(on_dev):
        def step():
            ok = C.c_int()
            if on_dev:
                rc = L.qg_kzg_verify_batch_dev(dev.h, C.byref(k), arr, n, None, C.byref(ok), None)
            else:
                rc = L.qg_kzg_verify_batch(C.byref(k), arr, n, None, C.byref(ok), None)
            assert rc == 0 and ok.value == 1, (rc, ok.value)
        return step

    fold(True)()  # warm the device path
    host_inner = inner if n <= (1 << 12) else 1
    res = {"claims": n, "msm_points": 2 * n + 1,
           "fold_host_ms": median_ms(fold(False), host_inner),
           "fold_device_ms": median_ms(fold(True), inner),
           "verify_host_ms": median_ms(verify(False), host_inner),
           "verify_device_ms": median_ms(verify(True), inner)}
    assert outs[True] == outs[False], "device fold differs from host fold"
    res["device_fold_faster"] = res["fold_device_ms"]["median"] < res["fold_host_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log", type=int, default=14)
    ap.add_argument("--ns", default="4,16,64,1024,16384")
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import quill_amd as q
    dev = q.Device(0)
    ns = [int(s) for s in args.ns.split(",")]
    out = {"inner": args.inner, "hyperplonk": hyperplonk_case(q, dev, args.rows_log, args.inner)}
    vk = q.KZG.verifier(tau=TAU)
    claims = synthetic_claims(max(ns))
    out["fold"] = {str(n): fold_case(q, dev, vk, claims, n, args.inner) for n in ns}
    faster = [n for n in ns if out["fold"][str(n)]["device_fold_faster"]]
    out["device_fold_beats_host_from_n"] = min(faster) if faster else None
    dev.close()
    txt = json.dumps(out, indent=1, sort_keys=True)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
