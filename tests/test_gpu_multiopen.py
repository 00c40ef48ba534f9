"""The multi-point batch opening on the device.

Building blocks (qg_eq_multi_dev, qg_mle_eval_multi_dev, qg_lincomb_dev), value
for value against Python integers.  The kernels split x at lb bits with
lb = nvars below 8, 8 up to nvars = 17 and nvars / 2 from there, so the sizes
are 1, 2 and 7 (less than a block, no high table), 8 (one block, still none),
9 (two high entries: fewer than a tile's rows), 12 and 13 (eq_table_device's
own split threshold, several tiles) and 18 (lb = 9).  At 22 variables (4096
tiles: a block of the evaluation kernel loops over four) the references are
closed forms and the existing eq table.

The protocol: MultiOpenProof.prove is bit-exact against the restated prover
(tests/multiopen_restatement.py), every field and the final transcript state;
at 13 variables, where the restated prover is too slow, the restated verifier
accepts the device proof."""
import ctypes as C
import random

import numpy as np
import pytest

import multiopen_restatement as mo
import quill_oracle as o

pytestmark = pytest.mark.gpu
R = o.R_MOD
TAU = 0x48595045524C4F4E4B
DOMAIN = b"gpu_multiopen"
INVALID, UNSUPPORTED = -1, -4
KS = (1, 2, 11)


def _q():
    import quill_amd
    return quill_amd


_REF = {}


def _points(nvars):
    """11 points, their eq tables and weights, computed once per size: point 1
    repeats point 0, point 2 has 0/1 coordinates, point 3 is all zeros; weight
    1 is zero and weight 2 is r - 1"""
    if nvars not in _REF:
        rnd = random.Random(7700 + nvars)
        pts = [[rnd.randrange(R) for _ in range(nvars)] for _ in range(11)]
        pts[1] = list(pts[0])
        pts[2] = [rnd.randrange(2) for _ in range(nvars)]
        pts[3] = [0] * nvars
        w = [rnd.randrange(R) for _ in range(11)]
        w[1], w[2] = 0, R - 1
        _REF[nvars] = (pts, [o.fast_eq_eval_hypercube(nvars, p) for p in pts], w)
    return _REF[nvars]


# ---------------------------------------------------------------- building blocks
@pytest.mark.parametrize("nvars", [1, 2, 7, 8, 9, 12, 13])
def test_eq_multi_vs_integers(dev, nvars):
    pts, tabs, w = _points(nvars)
    for k in KS:
        got = dev.eq_multi_dev(pts[:k], w[:k])
        want = [sum(w[i] * tabs[i][x] for i in range(k)) % R for x in range(1 << nvars)]
        assert got.to_list() == want, k
        got.close()
    # weight 1 alone is zero: the zero table
    z = dev.eq_multi_dev(pts[1:2], w[1:2])
    assert z.to_list() == [0] * (1 << nvars)
    z.close()


@pytest.mark.parametrize("nvars", [1, 2, 7, 8, 9, 12, 13])
def test_mle_eval_multi_vs_integers(dev, nvars):
    q = _q()
    pts, tabs, _ = _points(nvars)
    rnd = random.Random(nvars)
    poly = [rnd.randrange(R) for _ in range(1 << nvars)]
    poly[0], poly[-1] = R - 1, 0
    vec = q.DeviceVec.from_list(dev, poly)
    want = [sum(a * b for a, b in zip(poly, t)) % R for t in tabs]
    if nvars <= 9:
        assert want == [o.mle_evaluate(poly, p) for p in pts]
    assert want[2] == poly[sum(b << j for j, b in enumerate(pts[2]))] and want[3] == poly[0]
    for k in KS:
        assert dev.mle_eval_multi(vec, pts[:k]) == want[:k], k
    # a longer buffer: only the first 2^nvars entries count
    if nvars > 1:
        assert dev.mle_eval_multi(vec, [p[:-1] for p in pts[:2]]) == \
            [o.mle_evaluate(poly[:1 << (nvars - 1)], p[:-1]) for p in pts[:2]]


def test_eq_and_eval_at_18_variables(dev):
    """lb = 9: two column chunks per row of the evaluation kernel"""
    q = _q()
    nvars = 18
    rnd = random.Random(18)
    pts = [[rnd.randrange(R) for _ in range(nvars)] for _ in range(2)]
    w = [rnd.randrange(R), R - 1]
    tabs = [o.fast_eq_eval_hypercube(nvars, p) for p in pts]
    got = dev.eq_multi_dev(pts, w)
    assert got.to_list() == [(w[0] * a + w[1] * b) % R for a, b in zip(*tabs)]
    vals = np.arange(1 << nvars, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    vec = q.DeviceVec.from_u64(dev, vals)
    want = [sum(int(v) * e for v, e in zip(vals, t)) % R for t in tabs]
    assert dev.mle_eval_multi(vec, pts) == want


def test_eq_multi_equals_eq_table_entry_for_entry(dev):
    rnd = random.Random(3)
    for nvars in (1, 7, 8, 12, 13, 18, 22):
        z = [rnd.randrange(R) for _ in range(nvars)]
        a = dev.eq_multi_dev([z], [1])
        b = dev.eq_table_dev(z)
        assert a.first_mismatch(b) == -1, nvars
        a.close()
        b.close()


def test_large_sizes_against_closed_forms(dev):
    """22 variables: sum_x eq(x, z) = 1 and sum_x x eq(x, z) = sum_j 2^j z_j, so
    the multilinear extension of x -> c x + d at z is c sum_j 2^j z_j + d (every
    entry of every tile counts); eq_multi of two points is the linear
    combination of their eq tables"""
    q = _q()
    nvars = 22
    N = 1 << nvars
    rnd = random.Random(22)
    pts = [[rnd.randrange(R) for _ in range(nvars)] for _ in range(11)]
    pts[4] = [rnd.randrange(2) for _ in range(nvars)]
    c, d = 0x1F3D5B79, 0xDEADBEEF12345
    vec = q.DeviceVec.from_u64(dev, np.arange(N, dtype=np.uint64) * np.uint64(c) + np.uint64(d))
    want = [(c * sum(zj << j for j, zj in enumerate(z)) + d) % R for z in pts]
    assert dev.mle_eval_multi(vec, pts) == want
    assert dev.mle_eval_multi(vec, pts[:1]) == want[:1]
    w = [rnd.randrange(R), rnd.randrange(R)]
    tabs = [dev.eq_table_dev(z) for z in pts[:2]]
    a = dev.eq_multi_dev(pts[:2], w)
    b = dev.lincomb_dev(tabs, w)
    assert a.first_mismatch(b) == -1
    for v in tabs + [a, b, vec]:
        v.close()


@pytest.mark.parametrize("P", [1, 3, 16])
def test_lincomb_vs_integers(dev, P):
    q = _q()
    rnd = random.Random(P)
    for n in (1, 300, 8192 + 5):
        cols = [[rnd.randrange(R) for _ in range(n)] for _ in range(P)]
        cols[0][0] = R - 1
        coeffs = [rnd.randrange(R) for _ in range(P)]
        coeffs[0] = R - 1
        if P > 1:
            coeffs[1] = 0
        if P > 2:
            coeffs[P - 1] = R - 1
        vecs = [q.DeviceVec.from_list(dev, c) for c in cols]
        got = dev.lincomb_dev(vecs, coeffs)
        assert got.to_list() == [sum(a * col[x] for a, col in zip(coeffs, cols)) % R
                                 for x in range(n)]
        # the same vector twice is not aliasing; all-zero coefficients give zeros
        z = dev.lincomb_dev([vecs[0]] * P, [0] * P)
        assert z.to_list() == [0] * n


def test_argument_limits(dev):
    q = _q()
    L = q.lib()
    nv = 4
    N = 1 << nv
    pts = q.field.fr_array([5] * (257 * nv))
    ws = q.field.fr_array([1] * 257)
    out, poly, short = q.DeviceVec(dev, N), q.DeviceVec(dev, N).fill_random(1), q.DeviceVec(dev, N - 1)
    res = np.zeros((257, 4), dtype=np.uint64)
    u = q.field.u64p

    def eq(k=1, nvars=nv, p=u(pts), w=u(ws), o_=out.h, ctx=dev.h):
        return L.qg_eq_multi_dev(ctx, p, w, k, nvars, o_)

    def ev(k=1, nvars=nv, n=N, p=u(pts), f=poly.h, r=u(res), ctx=dev.h):
        return L.qg_mle_eval_multi_dev(ctx, f, n, p, k, nvars, r)

    assert eq() == 0 and ev() == 0 and eq(k=256) == 0 and ev(k=256) == 0
    for bad in (dict(k=0), dict(k=257), dict(nvars=0), dict(nvars=nv + 1), dict(nvars=64),
                dict(p=None), dict(ctx=None)):
        assert eq(**bad) == INVALID, bad
        if "nvars" not in bad or bad["nvars"] != nv + 1:
            assert ev(**bad) == INVALID, bad
    assert eq(w=None) == INVALID and eq(o_=None) == INVALID and eq(o_=short.h) == INVALID
    assert ev(f=None) == INVALID and ev(r=None) == INVALID and ev(f=short.h) == INVALID
    assert ev(n=N - 1) == INVALID and ev(n=2 * N) == INVALID and ev(nvars=nv + 1, n=2 * N) == INVALID

    vecs = [q.DeviceVec(dev, N).fill_random(i) for i in range(17)]
    cs = q.field.fr_array([1] * 17)

    def lin(P=2, n=N, hs=None, c=u(cs), o_=out.h, ctx=dev.h):
        hs = hs if hs is not None else [v.h.value for v in vecs]
        arr = (C.c_void_p * 17)(*(hs + [None] * (17 - len(hs))))
        return L.qg_lincomb_dev(ctx, arr, c, P, n, o_)

    assert lin() == 0 and lin(P=16) == 0 and lin(n=1) == 0
    assert lin(P=0) == INVALID and lin(P=17) == INVALID and lin(n=0) == INVALID
    assert lin(n=N + 1) == INVALID and lin(c=None) == INVALID and lin(o_=None) == INVALID
    assert lin(ctx=None) == INVALID and lin(hs=[vecs[0].h.value, None]) == INVALID
    assert L.qg_lincomb_dev(dev.h, None, u(cs), 1, N, out.h) == INVALID
    # aliasing: the output is an input, or a view that overlaps one
    assert lin(o_=vecs[1].h) == INVALID
    big = q.DeviceVec(dev, 2 * N).fill_random(9)
    a, b = big.view(0, N), big.view(N - 1, N)
    assert lin(P=1, hs=[a.h.value], o_=b.h) == INVALID
    assert lin(P=1, hs=[a.h.value], o_=big.view(N, N).h) == 0


def test_sharded_context_is_unsupported():
    q = _q()
    L = q.lib()
    group = q.Device.loopback_group(2)
    d = q.Device(0)
    d.attach_loopback(group, 0)
    assert d.comm_info()["sharded"]
    nv = 3
    out, poly = q.DeviceVec(d, 1 << nv), q.DeviceVec(d, 1 << nv).fill_random(1)
    for fn in (lambda: d.eq_multi_dev([[1, 2, 3]], [1], out=out),
               lambda: d.mle_eval_multi(poly, [[1, 2, 3]]),
               lambda: d.lincomb_dev([poly], [1], out=out)):
        with pytest.raises(q.QuillGpuError) as e:
            fn()
        assert e.value.code == UNSUPPORTED and "single context" in str(e.value)
    with pytest.raises(ValueError, match="sharded"):
        q.MultiOpenProof.prove([poly], [(0, [1, 2, 3])], q.KZG(d, None, 8, TAU),
                               q.Transcript(DOMAIN))
    out.close()
    poly.close()
    d.close()
    L.qg_loopback_destroy(group)


def test_entries_run_under_timed_regions(dev):
    q = _q()
    v = q.DeviceVec(dev, 16).fill_random(2)
    dev.enable_timing(True)
    try:
        before = {n: dev.kernel_time(n)[1] for n in ("eq_multi", "mle_eval_multi", "lincomb")}
        g = dev.eq_multi_dev([[1, 2, 3, 4]], [1])
        dev.mle_eval_multi(v, [[1, 2, 3, 4]])
        dev.lincomb_dev([v, g], [1, 2]).close()
        for n, c in before.items():
            ms, cnt = dev.kernel_time(n)
            assert cnt == c + 1 and ms > 0, n
        split = dev.phase_split(["eq_multi", "mle_eval_multi", "lincomb"])
        assert all(x > 0 for x in split.values())
    finally:
        dev.enable_timing(False)


# ---------------------------------------------------------------- the protocol
def _device_case(dev, n, P, k, seed=None):
    q = _q()
    polys, claims = mo.make_case(n, P, k, seed)
    pcs = q.KZG.trusted_setup(1 << n, TAU, dev)
    vecs = [q.DeviceVec.from_list(dev, f) for f in polys]
    return polys, claims, pcs, vecs


@pytest.mark.parametrize("P,k", [(1, 1), (3, 5), (5, 6)])
@pytest.mark.parametrize("n", [1, 3, 6])
def test_prove_bit_exact_vs_restatement(dev, n, P, k):
    q = _q()
    polys, claims, pcs, vecs = _device_case(dev, n, P, k)
    okzg = o.KZG(1 << n, TAU, points=[])
    ot = o.Transcript(DOMAIN)
    want = mo.prove(polys, claims, okzg, ot)
    generic = dev.counter("sc_generic_calls")
    t = q.Transcript(DOMAIN)
    proof = pcs.open_multi(vecs, claims, t)
    # 2P tables: the compiled sumcheck up to P = 4, the interpreter beyond
    assert dev.counter("sc_generic_calls") - generic == (1 if P > 4 else 0)
    assert mo.from_product(proof) == want
    assert t.state == ot.state
    # the inputs are untouched, and the product's verifier ends in the same state
    assert [v.to_list() for v in vecs] == polys
    vt = q.Transcript(DOMAIN)
    proof.verify([pcs.commit(v) for v in vecs], claims, pcs, vt)
    assert vt.state == ot.state
    pcs.close()


def test_13_variables_restated_verifier_accepts(dev):
    q = _q()
    n, P, k = 13, 3, 11
    polys, claims, pcs, vecs = _device_case(dev, n, P, k)
    t = q.Transcript(DOMAIN)
    proof = q.MultiOpenProof.prove(vecs, claims, pcs, t)
    assert proof.evaluations[2] == polys[claims[2][0]][sum(b << j
                                                          for j, b in enumerate(claims[2][1]))]
    comms = [pcs.commit(v) for v in vecs]
    ot = o.Transcript(DOMAIN)
    mo.verify(mo.from_product(proof), comms, claims, o.KZG(1 << n, TAU, points=[]), ot)
    assert ot.state == t.state
    vt = q.Transcript(DOMAIN)
    proof.verify(comms, claims, pcs, vt)
    assert vt.state == t.state
    back = q.deserialize(q.MultiOpenProof, q.serialize(proof))
    assert back == proof
    back.evaluations[7] = (back.evaluations[7] + 1) % R
    with pytest.raises(ValueError, match="Multi-open claimed sum mismatch"):
        back.verify(comms, claims, pcs, q.Transcript(DOMAIN))
    pcs.close()


def test_prove_refuses_a_polynomial_without_a_claim(dev):
    q = _q()
    _, claims, pcs, vecs = _device_case(dev, 3, 3, 5)
    with pytest.raises(AssertionError, match="without a claim"):
        q.MultiOpenProof.prove(vecs, [c for c in claims if c[0] != 1], pcs, q.Transcript(DOMAIN))
    pcs.close()
