"""InnerProductProof::prove on sharded contexts (qg_ipa_prove_dev with a
communicator, ipa_prove_sharded): rank c of W passes f[cL, (c+1)L), g[cL, (c+1)L)
and the SRS shard at offset cL.  The proof and the final transcript state on
every rank must equal, bit for bit, what the single-context call returns for
the concatenated vectors from a separate plain context (that proof is pinned
to the restatement by tests/test_gpu_ipa.py; one case here repeats the
comparison against tests/ipa_restatement.py directly).

Ranks are host threads over the loopback communicator (run_ranks).  The
switches (QG_IPA_PAIRED, QG_S_PRESUM_FUSED, QG_OPEN_CHECK) are read per call,
so the tests toggle them in-process around a whole group's run."""
import ctypes as C
import threading

import pytest

import ipa_restatement as ipa
import quill_oracle as o
from test_gpu_ipa import env, vec
from test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu
TAU = 0x5348415244495041
DOMAIN = b"gpu-ipa-sharded"
QNAMES = ("f at r", "f at 1/r", "g at r", "g at 1/r", "S at r", "S at 1/r")


# ---------------------------------------------------------------- helpers
_single = {}


def single(key, f, g):
    """(proof, state) of the single-context qg_ipa_prove_dev on a plain context
    of its own, computed once per key"""
    if key not in _single:
        import quill_amd as q
        dev0 = q.Device(0)
        kz = q.KZG.trusted_setup(len(f), TAU, dev0)
        df, dg = q.DeviceVec.from_list(dev0, f), q.DeviceVec.from_list(dev0, g)
        t = q.Transcript(DOMAIN)
        p = q.InnerProductProof.prove(df, dg, kz, t)
        df.close()
        dg.close()
        kz.close()
        dev0.close()
        _single[key] = (p, t.state)
    return _single[key]


def sharded(world, f, g, arm=None, shard_len=None):
    """every rank's (proof, state, open_checks delta, open_check_failures
    delta), or (error code, message).  arm(rank) -> (kind, value) or None;
    shard_len(rank): bases in that rank's SRS shard (default L).  No rank may
    be left in a collective: the thread count returns to its value before."""
    import quill_amd as q
    from quill_amd._lib import QuillGpuError
    L = len(f) // world
    assert len(f) == len(g) == world * L

    def fn(dev, rank, world):
        nb = shard_len(rank) if shard_len else L
        kzg = q.KZG(dev, q.Srs.generate(dev, TAU, nb, offset=rank * L), world * L - 1, TAU)
        df = q.DeviceVec.from_list(dev, f[rank * L:(rank + 1) * L])
        dg = q.DeviceVec.from_list(dev, g[rank * L:(rank + 1) * L])
        t = q.Transcript(DOMAIN)
        c0, f0 = dev.counter("open_checks"), dev.counter("open_check_failures")
        a = arm(rank) if arm else None
        if a:
            dev.debug_open_fault(*a)
        try:
            p = _prove(kzg, df, dg, L, t)
            res = (p, t.state, dev.counter("open_checks") - c0,
                   dev.counter("open_check_failures") - f0)
        except QuillGpuError as e:
            res = (e.code, str(e))
        df.close()
        dg.close()
        kzg.srs.close()
        return res
    before = threading.active_count()
    out = run_ranks(world, fn)
    assert threading.active_count() == before  # no rank is stuck in a collective
    return out


def _prove(kzg, df, dg, L, t):
    """qg_ipa_prove_dev against kzg's own SRS handle (whatever its length)"""
    import quill_amd as q
    from quill_amd._lib import IpaProof, check, lib
    from quill_amd.field import fr_from_mont_limbs, g1_from_abi
    from quill_amd.pcs import _IPA_OPENINGS, _opening
    out = IpaProof()
    check(lib().qg_ipa_prove_dev(kzg.dev.h, kzg.srs.h, df.h, L, dg.h, L, t.c_state(),
                                 C.byref(out)), kzg.dev.h)
    return q.InnerProductProof(fr_from_mont_limbs(list(out.inner_product)),
                               g1_from_abi(out.s_comm_xy, out.s_comm_inf),
                               *[_opening(getattr(out, n)) for n in _IPA_OPENINGS])


def assert_parity(out, want, checks=None):
    wp, wstate = want
    for rank, res in enumerate(out):
        assert len(res) == 4, (rank, res)
        p, state, dc, dfail = res
        assert p.inner_product == wp.inner_product, rank
        assert p.s_comm == wp.s_comm, rank
        for nm in ipa.OPENINGS:
            a, b = getattr(p, nm), getattr(wp, nm)
            assert (a.x, a.y, a.proof) == (b.x, b.y, b.proof), (rank, nm)
        assert state == wstate, rank
        assert dfail == 0, rank
        if checks is not None:
            assert dc == checks, rank


# ---------------------------------------------------------------- parity over (world, L)
# (2, 1024): the B-point transform (B = 2 L) at the first two-pass geometry
SHAPES = [(1, 64), (2, 1), (2, 32), (4, 1), (4, 16), (8, 1), (8, 8), (2, 1024)]


@pytest.mark.parametrize("world,L", SHAPES)
def test_parity_with_the_single_context(world, L):
    """W = 1: the `alt` / `sh` special cases; L = 1: B = 2; ranks 0 and W/2 own
    a residue that is its own mirror (c == -c), the others do not; ntt_plan
    runs stages [0, min(10, logn)) in its first pass (NTT_LGT = 10), so the
    B-point transform needs two passes from B = 2^11 on: L = 1024 (world 2)."""
    M = world * L
    f, g = vec(M, 100 + M + world), vec(M, 200 + M + world)
    out = sharded(world, f, g)
    assert_parity(out, single(("shape", world, L), f, g), checks=6)


def test_parity_with_the_restatement():
    world, L = 4, 16
    f, g = vec(64, 300), vec(64, 301)
    t = o.Transcript(DOMAIN)
    want = ipa.prove(f, g, o.KZG(64, TAU, points=[]), t)
    for res in sharded(world, f, g):
        assert len(res) == 4, res
        assert (ipa.from_product(res[0]), res[1]) == (want, t.state)


# ---------------------------------------------------------------- trimmed lengths
Z64 = [0] * 64
TRIMS = {
    "f40": (vec(64, 310, live=40), vec(64, 311)),   # ends inside rank 2's slice
    "f48": (vec(64, 312, live=48), vec(64, 313)),   # a slice boundary
    "f49": (vec(64, 314, live=49), vec(64, 315)),   # one past it
    "f1": (vec(64, 316, live=1), vec(64, 317)),     # empty quotients of f
    "g3": (vec(64, 318), vec(64, 319, live=3)),     # only rank 0 nonzero
    "g0": (vec(64, 320), Z64),                      # S empty, identity commitments
    "f0": (Z64, vec(64, 321)),
}


@pytest.mark.parametrize("name", sorted(TRIMS))
def test_trimmed_lengths(name):
    f, g = TRIMS[name]
    want = single(("trim", name), f, g)
    out = sharded(4, f, g)
    assert_parity(out, want)
    if name in ("g0", "f0"):
        p = out[0][0]
        assert p.s_comm is None
        assert (p.s_opening.y, p.s_opening.proof) == (0, None)
        assert (p.s_opening_inv.y, p.s_opening_inv.proof) == (0, None)
    if name == "f1":
        assert out[0][0].f_opening.proof is None and out[0][0].g_opening.proof is not None


# ---------------------------------------------------------------- route switches
@pytest.mark.parametrize("world,L", [(2, 64), (4, 16)])
def test_paired_jobs_give_the_default_proofs(world, L):
    """QG_IPA_PAIRED=1: three suffix_horner<2> jobs instead of six single ones
    (64 local coefficients at world 2: past the serial scan's 32)"""
    M = world * L
    f, g = vec(M, 400 + world), vec(M, 410 + world)
    want = single(("paired", world), f, g)
    with env("QG_IPA_PAIRED", "1"):
        paired = sharded(world, f, g)
    with env("QG_IPA_PAIRED", "0"):
        plain = sharded(world, f, g)
    assert_parity(paired, want, checks=6)
    assert_parity(plain, want, checks=6)


@pytest.mark.parametrize("world,L", [(4, 16), (8, 8)])
def test_fused_presum_equals_four_launches(world, L):
    """k_s_presum_fg (default) against k_s_presum per operand and residue
    (QG_S_PRESUM_FUSED=0): the same proofs, on ranks with c == -c (two outputs)
    and c != -c (four)"""
    M = world * L
    f, g = vec(M, 420 + world), vec(M, 430 + world)
    want = single(("presum", world), f, g)
    with env("QG_S_PRESUM_FUSED", "0"):
        four = sharded(world, f, g)
    with env("QG_S_PRESUM_FUSED", "1"):
        fused = sharded(world, f, g)
    assert_parity(four, want)
    assert_parity(fused, want)


# ---------------------------------------------------------------- the quotient check
def test_six_quotients_are_counted_on_every_rank():
    f, g = vec(64, 300), vec(64, 301)
    want = single("restated-shape", f, g)
    assert_parity(sharded(4, f, g), want, checks=6)
    with env("QG_OPEN_CHECK", "0"):
        assert_parity(sharded(4, f, g), want, checks=0)


@pytest.mark.parametrize("world,arm", [(4, lambda r: (2, 3) if r == 1 else None),
                                       (4, lambda r: (1, 5) if r == 3 else None),
                                       (2, lambda r: (2, 3) if r == 1 else None),
                                       (2, lambda r: (1, 5) if r == 1 else None)],
                         ids=["w4-quotient-rank1", "w4-short-trim-top", "w2-quotient-rank1",
                              "w2-short-trim-top"])
def test_fault_on_one_rank_fails_every_rank(world, arm):
    M = 64
    f, g = vec(M, 500), vec(M, 501)
    out = sharded(world, f, g, arm=arm)
    for res in out:
        assert len(res) == 2, res
        code, msg = res
        assert code == -5
        assert "Polynomial division failed" in msg
        assert any("(%s)" % n in msg for n in QNAMES), msg


# ---------------------------------------------------------------- statuses
def test_statuses_on_one_attached_rank():
    """geometry and emptiness are decided from the rank's own arguments, before
    the first collective: only rank 0 of a two-rank group is attached, so a
    call that entered a collective would never return"""
    import quill_amd as q
    from quill_amd._lib import IpaProof, QuillGpuError, lib
    from quill_amd.field import fr_array, u64p
    lb = lib()
    group = q.Device.loopback_group(2)
    d = q.Device(0)
    d.attach_loopback(group, 0)
    assert d.comm_info()["sharded"]
    srs = q.Srs.generate(d, TAU, 8)
    da, db = q.DeviceVec.from_list(d, vec(8, 600)), q.DeviceVec.from_list(d, vec(8, 601))
    out = IpaProof()
    st = q.Transcript(DOMAIN).c_state()

    def devc(nf, ng):
        return lb.qg_ipa_prove_dev(d.h, srs.h, da.h, nf, db.h, ng, st, C.byref(out))

    def last():
        m = lb.qg_last_error(d.h)
        return m.decode() if m else ""

    assert devc(4, 2) == -4 and "nf == ng" in last()
    assert devc(4, 0) == -4 and "nf == ng" in last()
    assert devc(3, 3) == -4 and "power of two" in last()   # 2 * 3
    assert devc(0, 0) == -1
    assert devc(9, 8) == -1 and devc(8, 9) == -1            # a length beyond the buffer
    # the host-pointer entry stays single-context
    a = fr_array([1, 2, 3, 4])
    assert lb.qg_ipa_prove(d.h, srs.h, u64p(a), 4, u64p(a), 4, st, C.byref(out)) == -4
    assert "sharded" in last()
    # ... and so does the Python mirror: host or mixed operands raise
    kzg = q.KZG(d, srs, 15, TAU)
    assert d.world == 2
    with pytest.raises(QuillGpuError) as e:
        q.InnerProductProof.prove([1, 2, 3, 4], [5, 6, 7, 8], kzg, q.Transcript(DOMAIN))
    assert e.value.code == -4 and "sharded" in str(e.value)
    with pytest.raises(QuillGpuError):
        q.InnerProductProof.prove(da, [5, 6, 7, 8], kzg, q.Transcript(DOMAIN))
    for x in (da, db, kzg):
        x.close()
    d.close()
    lb.qg_loopback_destroy(group)


@pytest.mark.parametrize("short", ["every rank", "rank 1 only"])
def test_shard_too_short_fails_every_rank(short):
    """16 local coefficients against 8 bases: -1 "Polynomial degree exceeds max
    degree" - on every rank, also when only one rank's shard is short (the
    shard sizes travel with the local lengths)"""
    f, g = vec(32, 610), vec(32, 611)
    out = sharded(2, f, g, shard_len=lambda r: 8 if (short == "every rank" or r == 1) else 16)
    for res in out:
        assert len(res) == 2, res
        assert res[0] == -1 and "Polynomial degree exceeds max degree" in res[1]


# ---------------------------------------------------------------- shared quotient stage
@pytest.mark.parametrize("order", ["openings first", "ipa first"])
def test_ml_openings_and_ipa_on_the_same_contexts(order):
    """a sharded ML opening batch of two items (world 4, nv = 6) and a sharded
    inner-product argument (L = 16) on the same contexts, in both orders: each
    equals its single-context counterpart, so the quotient stage's scratch
    slots, which both protocols use, carry nothing from one into the other"""
    import random
    import quill_amd as q
    world, nv, L = 4, 6, 16
    N = 1 << nv
    rnd = random.Random(910)
    polys = [[rnd.randrange(o.R_MOD) for _ in range(N)],
             [rnd.randrange(o.R_MOD) for _ in range(40)] + [0] * (N - 40)]
    pts = [[rnd.randrange(o.R_MOD) for _ in range(nv)] for _ in polys]
    f, g = vec(N, 911, live=N - 5), vec(N, 912)
    dev0 = q.Device(0)
    kz = q.KZG.trusted_setup(N, TAU, dev0)
    vs = [q.DeviceVec.from_list(dev0, p) for p in polys]
    t_ref = q.Transcript(DOMAIN)
    want_open = (kz.open_batch_dev([(v, N, pt, False) for v, pt in zip(vs, pts)], t_ref),
                 t_ref.state)
    for x in vs + [kz]:
        x.close()
    dev0.close()
    want_ipa = single("shared-stage", f, g)

    def fn(dev, rank, world):
        kzg = q.KZG.trusted_setup(N - 1, TAU, dev)
        vecs = [q.DeviceVec.from_list(dev, p[rank * L:(rank + 1) * L]) for p in polys]
        df = q.DeviceVec.from_list(dev, f[rank * L:(rank + 1) * L])
        dg = q.DeviceVec.from_list(dev, g[rank * L:(rank + 1) * L])

        def openings():
            t = q.Transcript(DOMAIN)
            return kzg.open_batch_dev([(v, L, pt, False) for v, pt in zip(vecs, pts)], t), t.state

        def argument():
            t = q.Transcript(DOMAIN)
            return q.InnerProductProof.prove(df, dg, kzg, t), t.state
        if order == "openings first":
            res = (openings(), argument())
        else:
            res = tuple(reversed((argument(), openings())))
        for x in vecs + [df, dg, kzg]:
            x.close()
        return res
    for got_open, got_ipa in run_ranks(world, fn):
        assert got_open == want_open
        assert got_ipa == want_ipa


# ---------------------------------------------------------------- Python mirror, verifier
def test_verifier_accepts_a_sharded_proof():
    """W = 8, L = 2^12 through InnerProductProof.prove(DeviceVec, DeviceVec, kzg, t)
    with kzg wrapping the SRS shard; the commitments come from the sharded MSM;
    qg_ipa_verify (pairings) accepts in the prover's transcript state, and the
    proof is the single-context one"""
    import quill_amd as q
    world, L = 8, 1 << 12
    M = world * L
    f, g = vec(M, 700), vec(M, 701)
    want, want_state = single("verifier", f, g)

    def fn(dev, rank, world):
        kzg = q.KZG(dev, q.Srs.generate(dev, TAU, L, offset=rank * L), M - 1, TAU)
        df = q.DeviceVec.from_list(dev, f[rank * L:(rank + 1) * L])
        dg = q.DeviceVec.from_list(dev, g[rank * L:(rank + 1) * L])
        c1, c2 = kzg.srs.msm_dev(df), kzg.srs.msm_dev(dg)
        t = q.Transcript(DOMAIN)
        p = q.InnerProductProof.prove(df, dg, kzg, t)
        df.close()
        dg.close()
        kzg.srs.close()
        return p, t.state, c1, c2
    out = run_ranks(world, fn)
    for p, state, c1, c2 in out:
        assert (p, state) == (want, want_state)
        assert (c1, c2) == out[0][2:]
    p, state, c1, c2 = out[0]
    vt = q.Transcript(DOMAIN)
    assert p.verify(c1, c2, q.KZG.verifier(TAU), vt)
    assert vt.state == state


# ---------------------------------------------------------------- forced RCCL
def test_forced_rccl_matches_single():
    """the sharded flow at world 1 over a real one-rank RCCL communicator
    (QG_FORCE_RCCL=1, as tests/test_gpu_rccl.py): allgathers and the S
    polynomial's all-to-all through RCCL; equal to the plain context's proof"""
    import quill_amd as q
    with env("QG_FORCE_RCCL", "1"):
        d = q.Device(0)
        d.attach_comm(0, 1, q.Device.comm_unique_id())
    assert d.comm_info() == {"kind": "rccl", "rank": 0, "world": 1, "sharded": True}
    n = 1 << 10
    f, g = vec(n, 800, live=n - 37), vec(n, 801)
    kzg = q.KZG(d, q.Srs.generate(d, TAU, n), n - 1, TAU)
    df, dg = q.DeviceVec.from_list(d, f), q.DeviceVec.from_list(d, g)
    t = q.Transcript(DOMAIN)
    p = q.InnerProductProof.prove(df, dg, kzg, t)
    for x in (df, dg, kzg.srs):
        x.close()
    d.close()
    assert (p, t.state) == single("rccl", f, g)
