"""The folded inner-product argument on the device.

  * the two-point evaluation kernel (qg_poly_eval2_dev) against qg_poly_eval_dev
    per polynomial and point, bit for bit, at the strip and span edges of the
    kernel (strip 32, span 8192), with the grid-stride loop wrapped
    (QG_EVAL_BLOCKS=1) and at the operand edges of x, and - both being
    instances of one kernel - against the oracle's Horner at the same edges;
  * qg_ipa_prove_folded[_dev] against the restatement
    (tests/foldipa_restatement.py), proof and transcript state bit for bit, on
    every route: QG_FOLD_FUSED unset / 1 and QG_EVAL_PAIRED 0 / 1;
  * trims, the quotient check's counters and the test faults, verification of
    device proofs, the launch counts (MSMs 7 -> 3), the statuses, and the plain
    paths untouched by a folded call on the same context.
The switches are read per call, so the tests toggle them in-process."""
import contextlib
import ctypes as C
import os
import random
import threading

import pytest

import foldipa_restatement as fi
import quill_oracle as o

pytestmark = pytest.mark.gpu
R = o.R_MOD
TAU = 0x464F4C44495041
DOMAIN = b"gpu_foldipa"
INVALID, UNSUPPORTED, ASSERT = -1, -4, -5
NMAX = 2 * 8192 + 1


def _q():
    import quill_amd
    return quill_amd


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


@pytest.fixture(scope="module")
def kzg(dev):
    k = _q().KZG.trusted_setup(2050, TAU, dev)
    yield k
    k.close()


# ---------------------------------------------------------------- two-point evaluation
@pytest.fixture(scope="module")
def srcs(dev):
    """eight random vectors of the largest length; a shorter one is a stated length"""
    q = _q()
    vs = [q.DeviceVec(dev, NMAX).fill_random(0xE7A10 + j) for j in range(8)]
    yield vs
    for v in vs:
        v.close()


LENGTHS = [0, 1, 31, 32, 33, 8191, 8192, 8193, NMAX]
_RND = random.Random(0xE7A12)
_RX = _RND.randrange(2, R)
XPAIRS = {"0,1": (0, 1), "p-1,random": (R - 1, _RND.randrange(2, R)),
          "r,1/r": (_RX, o.fr_inv(_RX)), "random,0": (_RND.randrange(2, R), 0)}
_SINGLE = {}


def single(srcs, j, n, x):
    """qg_poly_eval_dev of source j over n coefficients at x, computed once"""
    if (j, n, x) not in _SINGLE:
        _SINGLE[(j, n, x)] = srcs[j].evaluate(x, n)
    return _SINGLE[(j, n, x)]


def check_eval2(dev, srcs, lens, xs):
    P = len(lens)
    got = dev.poly_eval2(srcs[:P], lens, xs)
    want = [[single(srcs, j, lens[j], x) for j in range(P)] for x in xs]
    assert got == want, (lens, xs)


@pytest.mark.parametrize("xs", list(XPAIRS))
def test_eval2_one_polynomial_at_every_edge(dev, srcs, xs):
    for n in LENGTHS:
        check_eval2(dev, srcs, [n], XPAIRS[xs])


# unequal lengths in one call; together the P = 8 rows hold every length
MIXED = [(8193, 31, 0), (33, NMAX, 8192), (1, 32, 8191),
         (0, 1, 31, 32, 33, 8191, 8192, 8193), (NMAX, 8193, 8192, 8191, 33, 32, 31, 1)]


@pytest.mark.parametrize("xs", ["r,1/r", "p-1,random"])
@pytest.mark.parametrize("lens", MIXED, ids=["P%d-%d" % (len(m), i) for i, m in enumerate(MIXED)])
def test_eval2_unequal_lengths_in_one_call(dev, srcs, lens, xs):
    check_eval2(dev, srcs, list(lens), XPAIRS[xs])


def test_eval2_is_the_oracles_horner(dev, srcs):
    coeffs = srcs[0].to_list(33)
    xs = XPAIRS["r,1/r"]
    assert dev.poly_eval2(srcs[:1], [33], xs) == [[o.poly_eval(coeffs, x)] for x in xs]


@pytest.mark.parametrize("xs", ["r,1/r", "p-1,random"])
def test_eval2_matches_oracle_horner(dev, srcs, xs):
    """independent of qg_poly_eval_dev, which is an instance of the same kernel"""
    import oracle_c as oc
    arr = srcs[0].to_numpy()
    for n in LENGTHS:
        want = [[oc.fr_horner(arr[:n], x) if n else 0] for x in XPAIRS[xs]]
        assert dev.poly_eval2(srcs[:1], [n], XPAIRS[xs]) == want, n


def test_eval2_grid_stride_wraps(dev, srcs):
    """one block walks every span of the three longest lengths"""
    with env(QG_EVAL_BLOCKS="1"):
        for n in LENGTHS[-3:]:
            check_eval2(dev, srcs, [n], XPAIRS["r,1/r"])
        check_eval2(dev, srcs, LENGTHS[-3:], XPAIRS["p-1,random"])


def test_eval2_argument_limits(dev, srcs):
    L = _q().lib()
    hs = (C.c_void_p * 9)(*[srcs[0].h.value] * 9)
    ls = (C.c_size_t * 9)(*[8] * 9)
    xs = (C.c_uint64 * 8)()
    out = (C.c_uint64 * 72)()
    call = L.qg_poly_eval2_dev
    assert call(dev.h, hs, ls, 0, xs, out) == INVALID
    assert call(dev.h, hs, ls, 9, xs, out) == INVALID
    assert call(dev.h, None, ls, 1, xs, out) == INVALID
    assert call(dev.h, hs, None, 1, xs, out) == INVALID
    assert call(dev.h, hs, ls, 1, None, out) == INVALID
    assert call(dev.h, hs, ls, 1, xs, None) == INVALID
    assert call(None, hs, ls, 1, xs, out) == INVALID
    assert call(dev.h, (C.c_void_p * 2)(srcs[0].h.value, None), ls, 2, xs, out) == INVALID
    assert call(dev.h, hs, (C.c_size_t * 2)(8, NMAX + 1), 2, xs, out) == INVALID
    assert call(dev.h, hs, ls, 8, xs, out) == 0


# ---------------------------------------------------------------- prover parity
def vec(n, seed, live=None):
    rnd = random.Random(seed)
    live = n if live is None else live
    return [rnd.randrange(1, R) if i < live else 0 for i in range(n)]


# (33,33), (1025,1000), (2049,2049): across the scan's chunk edges (chunk length
# 32: one chunk row, two levels, three levels)
SIZES = [(1, 1), (2, 2), (3, 5), (33, 33), (33, 17), (64, 0), (0, 64), (1025, 1000),
         (2049, 2049)]
_RESTATED = {}


def operands(nf, ng):
    return vec(nf, 1000 * nf + ng), vec(ng, 1000 * ng + nf + 7)


def restated(f, g):
    """(proof, final transcript state) of the restated prover, computed once"""
    key = (tuple(f), tuple(g))
    if key not in _RESTATED:
        t = o.Transcript(DOMAIN)
        _RESTATED[key] = (fi.prove(f, g, o.KZG(2050, TAU, points=[]), t), t.state)
    return _RESTATED[key]


def device_prove(kzg, f, g, host=False):
    q = _q()
    t = q.Transcript(DOMAIN)
    if host:
        return fi.from_product(q.FoldedInnerProductProof.prove(f, g, kzg, t)), t.state
    # (an empty operand: a one-entry buffer, stated length 0)
    df, dg = q.DeviceVec.from_list(kzg.dev, f or [0]), q.DeviceVec.from_list(kzg.dev, g or [0])
    try:
        return raw_prove_dev(kzg, df, len(f), dg, len(g), t), t.state
    finally:
        df.close()
        dg.close()


def raw_prove_dev(kzg, df, nf, dg, ng, t):
    """qg_ipa_prove_folded_dev on the first nf / ng entries"""
    q = _q()
    from quill_amd._lib import IpaProofFolded, check
    from quill_amd.field import fr_from_mont_limbs, g1_from_abi
    out = IpaProofFolded()
    check(q.lib().qg_ipa_prove_folded_dev(kzg.dev.h, kzg.srs.h, df.h, nf, dg.h, ng, t.c_state(),
                                          C.byref(out)), kzg.dev.h)
    return {"inner_product": fr_from_mont_limbs(list(out.inner_product)),
            "s_comm": g1_from_abi(out.s_comm_xy, out.s_comm_inf),
            "y": [fr_from_mont_limbs(list(out.y[i])) for i in range(6)],
            "w": g1_from_abi(out.w_xy, out.w_inf), "w_inv": g1_from_abi(out.w_inv_xy, out.w_inv_inf)}


@pytest.mark.parametrize("paired", ["0", "1"], ids=["single-eval", "paired-eval"])
@pytest.mark.parametrize("fused", [None, "1"], ids=["composition", "fused-scan"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_prover_equals_restatement(kzg, size, fused, paired):
    f, g = operands(*size)
    want = restated(f, g)
    with env(QG_FOLD_FUSED=fused, QG_EVAL_PAIRED=paired):
        got = device_prove(kzg, f, g)
    assert got == want
    if size == (1, 1):  # S empty, quotients empty
        assert got[0]["s_comm"] is None and got[0]["w"] is None and got[0]["w_inv"] is None


def test_default_route_and_host_operands(kzg):
    f, g = operands(33, 17)
    with env(QG_FOLD_FUSED=None, QG_EVAL_PAIRED=None):
        assert device_prove(kzg, f, g) == restated(f, g)
        assert device_prove(kzg, f, g, host=True) == restated(f, g)
        # ... and through the folding view, DeviceVec operands by the class method
        q = _q()
        df, dg = q.DeviceVec.from_list(kzg.dev, f), q.DeviceVec.from_list(kzg.dev, g)
        t = q.Transcript(DOMAIN)
        p = q.FoldedInnerProductProof.prove(df, dg, kzg.folding(), t)
        df.close()
        assert (fi.from_product(p), t.state) == restated(f, g)
        with pytest.raises(q.QuillGpuError):  # one operand on the host, one on the device
            q.FoldedInnerProductProof.prove(f, dg, kzg, t)
        dg.close()


TRIMS = {"f-tail-shorter": (vec(64, 1, live=20), vec(40, 2)),   # f's trimmed length below g's
         "f-tail-longer": (vec(64, 3, live=50), vec(40, 4)),
         "f-zero": ([0] * 64, vec(64, 5)),
         "both-zero": ([0] * 64, [0] * 33),
         # the S vector (63 entries) is longer than both trimmed operands
         "s-longer": (vec(64, 6, live=10), vec(64, 7, live=7))}


@pytest.mark.parametrize("paired", ["0", "1"], ids=["single-eval", "paired-eval"])
@pytest.mark.parametrize("trim", list(TRIMS))
def test_trims(kzg, trim, paired):
    f, g = TRIMS[trim]
    want = restated(f, g)
    with env(QG_EVAL_PAIRED=paired):
        got = device_prove(kzg, f, g)
    assert got == want
    if trim == "both-zero":
        assert got[0]["y"] == [0] * 6 and got[0]["w"] is None and got[0]["w_inv"] is None
        assert got[0]["s_comm"] is None and got[0]["inner_product"] == 0
    if trim == "f-zero":
        assert got[0]["y"][:2] == [0, 0] and got[0]["w"] is not None


# ---------------------------------------------------------------- checks and faults
@pytest.mark.parametrize("fused", [None, "1"], ids=["composition", "fused-scan"])
def test_open_checks_and_faults(dev, kzg, fused):
    q = _q()
    f, g = operands(1025, 1000)
    want = restated(f, g)
    okzg = o.KZG(2050, TAU, points=[])
    comms = (okzg.commit(f), okzg.commit(g))
    with env(QG_FOLD_FUSED=fused):
        c0, f0 = dev.counter("open_checks"), dev.counter("open_check_failures")
        assert device_prove(kzg, f, g) == want
        assert dev.counter("open_checks") == c0 + 2
        with env(QG_OPEN_CHECK="0"):
            assert device_prove(kzg, f, g) == want
        assert dev.counter("open_checks") == c0 + 2
        assert dev.counter("open_check_failures") == f0
        for kind, value in ((2, 777), (1, 5)):
            dev.debug_open_fault(kind, value)
            with pytest.raises(q.QuillGpuError) as e:
                device_prove(kzg, f, g)
            assert e.value.code == ASSERT
            assert "Polynomial division failed" in str(e.value)
            assert "(folded at r)" in str(e.value) or "(folded at 1/r)" in str(e.value)
            assert device_prove(kzg, f, g) == want  # one-shot: the context is clean
        assert dev.counter("open_check_failures") > f0
        # without the check the fault goes through, and the host verifier rejects
        f1 = dev.counter("open_check_failures")
        with env(QG_OPEN_CHECK="0"):
            dev.debug_open_fault(2, 777)
            bad, state = device_prove(kzg, f, g)
        assert dev.counter("open_check_failures") == f1
        assert bad != want[0] and state == want[1]
        assert not fi.to_product(q, bad).verify(comms[0], comms[1], kzg, q.Transcript(DOMAIN))
        assert fi.to_product(q, want[0]).verify(comms[0], comms[1], kzg, q.Transcript(DOMAIN))


# ---------------------------------------------------------------- verification of device proofs
def test_device_proofs_verify(dev, kzg):
    q = _q()
    n = 2049
    df, dg = q.DeviceVec(dev, n).fill_random(0xD1), q.DeviceVec(dev, n).fill_random(0xD2)
    c1, c2 = kzg.commit(df), kzg.commit(dg)
    t = q.Transcript(DOMAIN)
    proof = q.FoldedInnerProductProof.prove(df, dg, kzg, t)
    df.close()
    dg.close()
    tv = q.Transcript(DOMAIN)
    assert proof.verify(c1, c2, kzg, tv) and tv.state == t.state
    view, tv = kzg.deferring(), q.Transcript(DOMAIN)
    assert proof.verify(c1, c2, view, tv) and tv.state == t.state
    assert len(view.claims) == 2
    view.check()  # one pairing check for both claims
    again = q.deserialize(q.FoldedInnerProductProof, q.serialize(proof))
    assert again == proof and again.verify(c1, c2, kzg, q.Transcript(DOMAIN))
    assert not proof.verify(c2, c1, kzg, q.Transcript(DOMAIN))
    view = kzg.deferring()
    proof.verify(c2, c1, view, q.Transcript(DOMAIN))
    with pytest.raises(ValueError):
        view.check()


# ---------------------------------------------------------------- neighbours untouched
def test_plain_paths_untouched(dev, kzg):
    """the scratch slots are shared: a plain inner-product proof and a folded ML
    opening before and after a folded inner-product proof are identical"""
    q = _q()
    f, g = operands(1025, 1000)
    poly, point = vec(1024, 77), vec(10, 78)
    pv = q.DeviceVec.from_list(dev, poly)

    def plain(view):
        t = q.Transcript(DOMAIN)
        return q.InnerProductProof.prove(f, g, view, t), t.state

    def folded_ml():
        t = q.Transcript(DOMAIN)
        return kzg.folding().open_dev(pv, len(poly), point, t), t.state
    before, before_ml = plain(kzg), folded_ml()
    assert isinstance(before[0], q.InnerProductProof)
    for fused in (None, "1"):
        for paired in ("0", "1"):
            with env(QG_FOLD_FUSED=fused, QG_EVAL_PAIRED=paired):
                device_prove(kzg, f, g)
    assert plain(kzg) == before
    assert plain(kzg.folding()) == before  # the view forwards: a plain proof
    assert folded_ml() == before_ml
    pv.close()


# ---------------------------------------------------------------- launch counts
def test_launch_counts(dev, kzg):
    """MSMs from the accumulate region's entry count, one entry per non-empty
    MSM of a batch: the plain proof commits S and six quotients, the folded one
    S and two; observed (7, 3).  fold_eval is entered once per folded proof."""
    q = _q()
    f, g = operands(33, 33)

    def entries(name):
        return dev.kernel_time(name)[1]
    dev.enable_timing(True)
    try:
        m0, e0 = entries("msm_accumulate"), entries("fold_eval")
        q.InnerProductProof.prove(f, g, kzg, q.Transcript(DOMAIN))
        m1, e1 = entries("msm_accumulate"), entries("fold_eval")
        device_prove(kzg, f, g)
        m2, e2 = entries("msm_accumulate"), entries("fold_eval")
    finally:
        dev.enable_timing(False)
    print("msm_accumulate entries (plain, folded):", (m1 - m0, m2 - m1))
    assert (m1 - m0, m2 - m1) == (7, 3)
    assert (e1 - e0, e2 - e1) == (0, 1)


# ---------------------------------------------------------------- limits
def test_limits(dev, kzg):
    q = _q()
    from quill_amd._lib import IpaProofFolded
    L = q.lib()
    v = q.DeviceVec.from_list(dev, vec(64, 90))
    out = IpaProofFolded()
    st = q.Transcript(DOMAIN).c_state()
    host = (C.c_uint64 * 4)()
    assert L.qg_ipa_prove_folded_dev(dev.h, kzg.srs.h, v.h, 0, v.h, 0, st, C.byref(out)) == INVALID
    assert L.qg_ipa_prove_folded(dev.h, kzg.srs.h, host, 0, host, 0, st, C.byref(out)) == INVALID
    assert L.qg_ipa_prove_folded_dev(dev.h, kzg.srs.h, v.h, 65, v.h, 1, st, C.byref(out)) == INVALID
    assert L.qg_ipa_prove_folded_dev(dev.h, kzg.srs.h, None, 1, v.h, 1, st, C.byref(out)) == INVALID
    assert L.qg_ipa_prove_folded_dev(dev.h, None, v.h, 1, v.h, 1, st, C.byref(out)) == INVALID
    assert L.qg_ipa_prove_folded(dev.h, kzg.srs.h, None, 1, host, 1, st, C.byref(out)) == INVALID
    v.close()
    # g empty: S is zero and L_h = 64, so the quotients commit over 63
    # coefficients: an SRS of 63 bases is enough, one of 62 is not
    f = vec(64, 91)
    for n, ok in ((63, True), (62, False)):
        small = q.KZG.trusted_setup(n - 1, TAU, dev)
        if ok:
            assert device_prove(small, f, []) == restated(f, [])
        else:
            with pytest.raises(q.QuillGpuError) as e:
                device_prove(small, f, [])
            assert e.value.code == INVALID and "Polynomial degree exceeds max degree" in str(e.value)
        small.close()
    # ... and S itself one base short
    f, g = operands(33, 33)
    small = q.KZG.trusted_setup(30, TAU, dev)
    with pytest.raises(q.QuillGpuError) as e:
        device_prove(small, f, g)
    assert e.value.code == INVALID and "Polynomial degree exceeds max degree" in str(e.value)
    small.close()


def test_sharded_context_is_unsupported():
    q = _q()
    from quill_amd._lib import IpaProofFolded
    L = q.lib()
    d = q.Device(0)
    srs = q.Srs.generate(d, TAU, 16)
    poly = q.DeviceVec(d, 8).fill_random(1)
    group = q.Device.loopback_group(1)
    d.attach_loopback(group, 0)
    assert d.comm_info()["sharded"]
    before = threading.active_count()
    st = (C.c_uint8 * 32)()
    out = IpaProofFolded()
    host = (C.c_uint64 * 32)()
    hs = (C.c_void_p * 1)(poly.h.value)
    ls = (C.c_size_t * 1)(8)
    for rc in (L.qg_ipa_prove_folded_dev(d.h, srs.h, poly.h, 8, poly.h, 8, st, C.byref(out)),
               L.qg_ipa_prove_folded(d.h, srs.h, host, 8, host, 8, st, C.byref(out)),
               L.qg_poly_eval2_dev(d.h, hs, ls, 1, host, host)):
        assert rc == UNSUPPORTED
        assert b"sharded" in L.qg_last_error(d.h)
    assert bytes(st) == bytes(32)  # before any transcript step
    with pytest.raises(ValueError, match="sharded"):
        q.FoldedInnerProductProof.prove(poly, poly, q.KZG(d, None, 8, TAU), q.Transcript(DOMAIN))
    assert threading.active_count() == before  # nobody waits in a collective
    poly.close()
    srs.close()
    d.close()
    L.qg_loopback_destroy(group)
