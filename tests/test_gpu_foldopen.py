"""The folded ML opening on the device.

  * the two-source suffix-Horner scan through qg_kzg_open_lincomb_dev against
    qg_lincomb_dev + download + qg_kzg_open, bit for bit, with QG_FOLD_FUSED
    unset, 0 (the unfused composition) and 1 (the fused scan), at lengths that cross every path of the recursion
    (chunk length 32: one thread, one chunk row, two levels, three levels);
  * operand edges (p - 1, 0, alternating, a cancelling pair);
  * qg_mle_open_folded_dev / _batch_dev against the restatement
    (tests/foldopen_restatement.py), proof and transcript state bit for bit;
  * a larger size through the product verifier;
  * the counts (MSMs 5 -> 3, KZG claims 4 -> 2 per opening), the quotient
    check's counters and the test faults, the statuses, and the plain path
    untouched by a folded call on the same context.
The switches are read per call, so the tests toggle them in-process."""
import contextlib
import ctypes as C
import os
import random

import numpy as np
import pytest

import foldopen_restatement as fo
import quill_oracle as o

pytestmark = pytest.mark.gpu
R = o.R_MOD
TAU = 0x464F4C444F50454E
DOMAIN = b"gpu_foldopen"
INVALID, UNSUPPORTED, ASSERT = -1, -4, -5
NMAX = (1 << 16) + 5


def _q():
    import quill_amd
    return quill_amd


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


@pytest.fixture(scope="module")
def kzg(dev):
    k = _q().KZG.trusted_setup(NMAX + 2, TAU, dev)
    yield k
    k.close()


@pytest.fixture(scope="module")
def srcs(dev):
    """four random vectors of the largest length; shorter sources are views"""
    q = _q()
    vs = [q.DeviceVec(dev, NMAX).fill_random(0xF01D0 + j) for j in range(4)]
    yield vs
    for v in vs:
        v.close()


# QG_FOLD_FUSED: unset (the default route: the unfused composition), 0 (the
# same, explicitly) and 1 (the fused scan)
FUSED, FUSED_IDS = [None, "0", "1"], ["unset", "unfused", "fused"]
_RND = random.Random(0xF01DED)
COEFFS = [_RND.randrange(1, R) for _ in range(4)]
XS = [_RND.randrange(1, R), _RND.randrange(1, R)]


def reference(dev, kzg, vecs, lens, coeffs, xs):
    """qg_lincomb_dev of the zero-padded sources, downloaded, qg_kzg_open per point"""
    q = _q()
    L = max(lens)
    padded = []
    for v, n in zip(vecs, lens):
        p = q.DeviceVec.from_u64(dev, np.zeros(L, dtype=np.uint64))
        if n:
            p.copy_from(v, n=n)
        padded.append(p)
    h = dev.lincomb_dev(padded, coeffs, n=L)
    hl = h.to_list()
    for p in padded + [h]:
        p.close()
    return [kzg.open_univariate(hl, x) for x in xs]


# (name, lens, first coefficient is 1): the lengths cross every path of the
# recursion; P = 2 with unequal lengths both ways and one source empty; P = 3, 4
GEOMETRY = [("L%d" % n, (n, n), True) for n in (1, 2, 32, 33, 63, 1024, 1025, 2049,
                                                 (1 << 15) + 1, NMAX)]
GEOMETRY += [("short1-33", (33, 17), True), ("short0-33", (17, 33), True),
             ("short1-1025", (1025, 40), True), ("short0-1025", (513, 1025), True),
             ("short0-2049", (1030, 2049), False),
             ("empty1-33", (33, 0), True), ("empty0-33", (0, 33), True),
             ("empty1-1025", (1025, 0), False), ("empty0-1025", (0, 1025), True),
             ("P3-33", (33, 20, 33), True), ("P3-1025", (1000, 1025, 64), True),
             ("P4-33", (33, 33, 1, 32), False), ("P4-1025", (1025, 1024, 1025, 31), True),
             ("P1-1025", (1025,), False)]
_REF = {}


@pytest.mark.parametrize("fused", FUSED, ids=FUSED_IDS)
@pytest.mark.parametrize("name,lens,one0", GEOMETRY, ids=[g[0] for g in GEOMETRY])
def test_scan_geometry(dev, kzg, srcs, name, lens, one0, fused):
    vecs = srcs[:len(lens)]
    coeffs = ([1] if one0 else [COEFFS[0]]) + COEFFS[1:len(lens)]
    if name not in _REF:
        _REF[name] = reference(dev, kzg, vecs, lens, coeffs, XS)
    want = _REF[name]
    with env("QG_FOLD_FUSED", fused):
        assert kzg.open_lincomb_dev(vecs, lens, coeffs, XS) == want
        # one point: the scan's NP = 1 form
        assert kzg.open_lincomb_dev(vecs, lens, coeffs, XS[1:]) == want[1:]


EDGES = ["pm1", "zero", "alt0", "alt1", "cancel"]


@pytest.mark.parametrize("fused", FUSED, ids=FUSED_IDS)
@pytest.mark.parametrize("n", [33, 64])
@pytest.mark.parametrize("kind", EDGES)
def test_operand_edges(dev, kzg, kind, n, fused):
    q = _q()
    rnd = random.Random(n)
    gamma = R - 1
    if kind == "pm1":
        a, b = [R - 1] * n, [R - 1] * n
    elif kind == "zero":
        a, b = [0] * n, [0] * n
    elif kind == "alt0":
        a, b = [(R - 1) * (i & 1) for i in range(n)], [(R - 1) * (~i & 1) for i in range(n)]
    elif kind == "alt1":
        a, b = [(R - 1) * (~i & 1) for i in range(n)], [(R - 1) * (~i & 1) for i in range(n)]
    else:  # source 1 is the negative of source 0, gamma = 1: h = 0
        a = [rnd.randrange(1, R) for _ in range(n)]
        b, gamma = [R - x for x in a], 1
    va, vb = q.DeviceVec.from_list(dev, a), q.DeviceVec.from_list(dev, b)
    key = (kind, n)
    if key not in _REF:
        _REF[key] = reference(dev, kzg, [va, vb], (n, n), [1, gamma], XS)
    with env("QG_FOLD_FUSED", fused):
        got = kzg.open_lincomb_dev([va, vb], (n, n), [1, gamma], XS)
    va.close()
    vb.close()
    assert got == _REF[key]
    h = [(x + gamma * y) % R for x, y in zip(a, b)]
    assert [g.y for g in got] == [o.poly_eval(h, x) for x in XS]
    if kind in ("zero", "cancel"):
        assert all(g.y == 0 and g.proof is None for g in got)


# ---------------------------------------------------------------- prover parity
def restated(poly, point, nv):
    okzg = o.KZG(1 << nv, TAU, points=[])
    t = o.Transcript(DOMAIN)
    return fo.prove(poly, point, okzg, t), t.state


def device_open(kzg, vec, n, point, **kw):
    q = _q()
    t = q.Transcript(DOMAIN)
    p = kzg.folding().open_dev(vec, n, point, t, **kw)
    return fo.from_product(p), t.state


def case(nv, seed=0):
    rnd = random.Random(1000 * nv + seed)
    return ([rnd.randrange(R) for _ in range(1 << nv)], [rnd.randrange(R) for _ in range(nv)])


@pytest.mark.parametrize("fused", FUSED, ids=FUSED_IDS)
@pytest.mark.parametrize("nv", [1, 2, 5, 6, 10, 11])
def test_prover_equals_restatement(dev, kzg, nv, fused):
    q = _q()
    poly, point = case(nv)
    if ("prove", nv) not in _REF:
        _REF[("prove", nv)] = restated(poly, point, nv)
    vec = q.DeviceVec.from_list(dev, poly)
    with env("QG_FOLD_FUSED", fused):
        got = device_open(kzg, vec, len(poly), point)
    vec.close()
    assert got == _REF[("prove", nv)]


def test_batch_of_three(dev, kzg):
    q = _q()
    nv = 6
    cases = [case(nv, s) for s in (1, 2, 3)]
    vecs = [q.DeviceVec.from_list(dev, p) for p, _ in cases]
    okzg = o.KZG(1 << nv, TAU, points=[])
    ot = o.Transcript(DOMAIN)
    want = [fo.prove(p, pt, okzg, ot) for p, pt in cases]
    t = q.Transcript(DOMAIN)
    got = kzg.folding().open_batch_dev([(v, 1 << nv, pt, False)
                                        for v, (_, pt) in zip(vecs, cases)], t)
    t1 = q.Transcript(DOMAIN)
    single = [kzg.folding().open_dev(v, 1 << nv, pt, t1) for v, (_, pt) in zip(vecs, cases)]
    for v in vecs:
        v.close()
    assert got == single and t.state == t1.state == ot.state
    assert [fo.from_product(p) for p in got] == want


TRIMS = {"n40": lambda p: p[:40],                                # S is longer than f
         "live40": lambda p: p[:40] + [0] * 24,
         "live1": lambda p: p[:1] + [0] * 63,                    # f's own quotient is empty
         "zero": lambda p: [0] * 64}


@pytest.mark.parametrize("trim", list(TRIMS))
def test_trims(dev, kzg, trim):
    q = _q()
    poly, point = case(6, 9)
    poly = TRIMS[trim](poly)
    want = restated(poly, point, 6)
    vec = q.DeviceVec.from_list(dev, poly)
    got = device_open(kzg, vec, len(poly), point)
    vec.close()
    assert got == want
    if trim == "zero":
        assert got[0]["y"] == [0] * 4 and got[0]["w"] is None and got[0]["w_inv"] is None
    if trim == "live1":
        assert got[0]["w"] is not None


def test_unchanged_flag_gives_the_same_proofs(dev, kzg):
    q = _q()
    poly, point = case(10, 4)
    _, point2 = case(10, 5)
    vec = q.DeviceVec.from_list(dev, poly)
    a = device_open(kzg, vec, len(poly), point)
    b = device_open(kzg, vec, len(poly), point2)
    assert device_open(kzg, vec, len(poly), point, unchanged=True) == a
    assert device_open(kzg, vec, len(poly), point2, unchanged=True) == b
    vec.close()


def test_larger_size_verifies(dev, kzg):
    q = _q()
    nv = 16
    vec = q.DeviceVec(dev, 1 << nv).fill_random(0x16)
    point = case(nv)[1]
    comm = kzg.commit(vec)
    t = q.Transcript(DOMAIN)
    proof = kzg.folding().open_dev(vec, 1 << nv, point, t)
    vec.close()
    tv = q.Transcript(DOMAIN)
    assert proof.verify(comm, kzg, tv) and tv.state == t.state
    view, tv = kzg.deferring(), q.Transcript(DOMAIN)
    assert proof.verify(comm, view, tv) and tv.state == t.state
    view.check()
    assert not proof.verify(kzg.commit([1, 2, 3]), kzg, q.Transcript(DOMAIN))


# ---------------------------------------------------------------- counts, counters, faults
def test_counts_per_opening(dev, kzg):
    """MSMs 5 -> 3 (so quotient vectors, each committed by one MSM beside S's,
    4 -> 2) from the accumulate region's launch count; KZG claims 4 -> 2"""
    q = _q()
    poly, point = case(10, 6)
    vec = q.DeviceVec.from_list(dev, poly)
    comm = kzg.commit(vec)

    def msms():
        return dev.kernel_time("msm_accumulate")[1]
    dev.enable_timing(True)
    try:
        m0 = msms()
        plain = kzg.open_dev(vec, len(poly), point, q.Transcript(DOMAIN))
        m1 = msms()
        folded = kzg.folding().open_dev(vec, len(poly), point, q.Transcript(DOMAIN))
        m2 = msms()
    finally:
        dev.enable_timing(False)
    vec.close()
    assert (m1 - m0, m2 - m1) == (5, 3)
    for proof, claims in ((plain, 4), (folded, 2)):
        view = kzg.deferring()
        assert proof.verify(comm, view, q.Transcript(DOMAIN))
        assert len(view.claims) == claims
        view.check()


@pytest.mark.parametrize("fused", [None, "1"], ids=["unset", "fused"])
def test_open_checks_and_faults(dev, kzg, monkeypatch, fused):
    q = _q()
    if fused is None:
        monkeypatch.delenv("QG_FOLD_FUSED", raising=False)
    else:
        monkeypatch.setenv("QG_FOLD_FUSED", fused)
    poly, point = case(10, 7)
    vec = q.DeviceVec.from_list(dev, poly)
    want = device_open(kzg, vec, len(poly), point)
    c0, f0 = dev.counter("open_checks"), dev.counter("open_check_failures")
    assert device_open(kzg, vec, len(poly), point) == want
    assert dev.counter("open_checks") == c0 + 2
    with env("QG_OPEN_CHECK", "0"):
        assert device_open(kzg, vec, len(poly), point) == want
    assert dev.counter("open_checks") == c0 + 2
    t = q.Transcript(DOMAIN)
    kzg.folding().open_batch_dev([(vec, len(poly), point, False)] * 3, t)
    assert dev.counter("open_checks") == c0 + 8
    assert dev.counter("open_check_failures") == f0
    for kind, value in ((2, 777), (1, 5)):
        dev.debug_open_fault(kind, value)
        with pytest.raises(q.QuillGpuError) as e:
            device_open(kzg, vec, len(poly), point)
        assert e.value.code == ASSERT
        assert "Polynomial division failed" in str(e.value) and "(folded at" in str(e.value)
        assert device_open(kzg, vec, len(poly), point) == want  # one-shot: the context is clean
    assert dev.counter("open_check_failures") > f0
    # the building block runs the same check
    c1 = dev.counter("open_checks")
    kzg.open_lincomb_dev([vec, vec], (1024, 1000), [1, 5], XS)
    assert dev.counter("open_checks") == c1 + 2
    dev.debug_open_fault(2, 3)
    with pytest.raises(q.QuillGpuError) as e:
        kzg.open_lincomb_dev([vec, vec], (1024, 1000), [1, 5], XS)
    assert e.value.code == ASSERT and "Polynomial division failed" in str(e.value)
    vec.close()


# ---------------------------------------------------------------- statuses
def test_sharded_context_is_unsupported_for_folded_entries():
    q = _q()
    from quill_amd._lib import KzgOpening, MleOpenItem, MleProofFolded
    L = q.lib()
    d = q.Device(0)
    srs = q.Srs.generate(d, TAU, 16)
    poly = q.DeviceVec(d, 8).fill_random(1)
    group = q.Device.loopback_group(1)
    d.attach_loopback(group, 0)
    assert d.comm_info()["sharded"]
    pt = (C.c_uint64 * 12)()
    st = (C.c_uint8 * 32)()
    out = (MleProofFolded * 1)()
    items = (MleOpenItem * 1)(MleOpenItem(poly.h.value, 8, pt, 3, 0, 0))
    hs = (C.c_void_p * 1)(poly.h.value)
    ls = (C.c_size_t * 1)(8)
    ops = (KzgOpening * 1)()
    for rc in (L.qg_mle_open_folded_dev(d.h, srs.h, poly.h, 8, pt, 3, st, 0, out),
               L.qg_mle_open_folded_batch_dev(d.h, srs.h, items, 1, st, out),
               L.qg_kzg_open_lincomb_dev(d.h, srs.h, hs, ls, pt, 1, pt, 1, ops)):
        assert rc == UNSUPPORTED
        assert b"sharded" in L.qg_last_error(d.h)
    assert bytes(st) == bytes(32)  # before any transcript step
    with pytest.raises(ValueError, match="sharded"):
        q.KZG(d, None, 8, TAU).folding()
    poly.close()
    srs.close()
    d.close()
    L.qg_loopback_destroy(group)


def test_degree_message_and_invalid_limits(dev, srcs):
    q = _q()
    from quill_amd._lib import KzgOpening
    L = q.lib()
    poly, point = case(6, 8)
    vec = q.DeviceVec.from_list(dev, poly)
    # S commits over 63 coefficients and the quotients over L_h - 1 = 63: an
    # SRS of 63 bases is enough, one of 62 is not
    for n, ok in ((63, True), (62, False)):
        small = q.KZG.trusted_setup(n - 1, TAU, dev)
        if ok:
            small.folding().open_dev(vec, 64, point, q.Transcript(DOMAIN))
        else:
            with pytest.raises(q.QuillGpuError) as e:
                small.folding().open_dev(vec, 64, point, q.Transcript(DOMAIN))
            assert e.value.code == INVALID and "Polynomial degree exceeds max degree" in str(e.value)
            with pytest.raises(q.QuillGpuError) as e:
                small.open_lincomb_dev([vec, vec], (64, 10), [1, 2], XS)
            assert e.value.code == INVALID and "Polynomial degree exceeds max degree" in str(e.value)
        small.close()
    big = q.KZG.trusted_setup(64, TAU, dev)
    hs = (C.c_void_p * 5)(*[vec.h.value] * 5)
    ls = (C.c_size_t * 5)(*[8] * 5)
    cs = (C.c_uint64 * 20)()
    ops = (KzgOpening * 3)()
    call = L.qg_kzg_open_lincomb_dev
    assert call(dev.h, big.srs.h, hs, ls, cs, 0, cs, 1, ops) == INVALID
    assert call(dev.h, big.srs.h, hs, ls, cs, 5, cs, 1, ops) == INVALID
    assert call(dev.h, big.srs.h, hs, ls, cs, 2, cs, 0, ops) == INVALID
    assert call(dev.h, big.srs.h, hs, ls, cs, 2, cs, 3, ops) == INVALID
    assert call(dev.h, big.srs.h, hs, (C.c_size_t * 2)(8, 65), cs, 2, cs, 1, ops) == INVALID
    assert call(dev.h, big.srs.h, None, ls, cs, 2, cs, 1, ops) == INVALID
    assert call(dev.h, big.srs.h, (C.c_void_p * 2)(vec.h.value, None), ls, cs, 2, cs, 1,
                ops) == INVALID
    assert call(dev.h, big.srs.h, hs, ls, cs, 2, cs, 1, ops) == 0
    big.close()
    vec.close()


# ---------------------------------------------------------------- the plain path
def test_plain_path_untouched(dev, kzg):
    """the scratch slots are shared: a plain opening before and after a folded
    call on the same context returns identical proofs"""
    q = _q()
    poly, point = case(10, 3)
    vec = q.DeviceVec.from_list(dev, poly)

    def plain():
        t = q.Transcript(DOMAIN)
        return kzg.open_dev(vec, len(poly), point, t), t.state
    before = plain()
    device_open(kzg, vec, len(poly), point)
    with env("QG_FOLD_FUSED", "1"):
        device_open(kzg, vec, len(poly), point)
        kzg.open_lincomb_dev([vec, vec], (1024, 77), [1, 5], XS)
    kzg.open_lincomb_dev([vec, vec], (1024, 77), [1, 5], XS)
    assert plain() == before
    # ... and it is the oracle's proof
    op = o.MLEvalProof.prove(poly, point, o.KZG(1 << 10, TAU, points=[]), o.Transcript(DOMAIN))
    assert (before[0].evaluation, before[0].s_comm) == (op.evaluation, op.s_comm)
    assert (before[0].poly_opening.x, before[0].poly_opening.y) == op.poly_opening[:2]
    vec.close()
