"""The column materialiser (qg_expr_column[_dev], csrc/logup.hip k_expr_column),
lookup_multiplicities(..., materialise=True) and LookupProof.prove over an
expression column.

The reference for the primitive is VirtualPolyExpr.evaluate row by row; the
device words must be the canonical Montgomery words of those values, bit for
bit.  The multiplicity column is a dict count written here."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

import quill_oracle as o

pytestmark = pytest.mark.gpu
R = o.R_MOD
TAU = 0x1234567890ABCDEF1122334455667788
U64P = C.POINTER(C.c_uint64)


def run_ranks(world, fn):
    import quill_amd as q
    group = q.Device.loopback_group(world)
    out = [None] * world
    err = []

    def body(rank):
        try:
            dev = q.Device(0)
            dev.attach_loopback(group, rank)
            out[rank] = fn(dev, rank, world)
            dev.close()
        except Exception as e:  # surfaced below
            err.append(e)

    ths = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=600)
    q.lib().qg_loopback_destroy(group)
    assert not err, err
    return out


def _exprs():
    """name -> (expression over tables a, b, c, d, e = 0 .. 4, tables it reads)"""
    from quill_amd import VirtualPolyExpr as E
    a, b, c, d, e = (E.Input(i) for i in range(5))
    return {
        "input": c,
        "const": E.Const(R - 5),
        "a_plus_1": a + E.Const(1),
        "ab_minus_c": a * b - c,
        "degree5": a * b * c * d * e,
        "scaled_factor": E.Const(0xDEADBEEF) * b,
        "packed": a + E.Const(256) * b,
        "mixed": (a + E.Const(3)) * (b - c) * a + E.Const(7) * d * d,
    }


def _tables(nvars, seed):
    """five tables of 2^nvars entries: random, with 0 and r - 1 among the inputs
    and, where there is room, rows at which a + 1 and a b - c are 0 mod r"""
    rnd = random.Random(seed)
    n = 1 << nvars
    tabs = [[rnd.randrange(R) for _ in range(n)] for _ in range(5)]
    tabs[0][0] = R - 1                       # a + 1 == 0 at row 0
    if n > 1:
        tabs[2][1] = tabs[0][1] * tabs[1][1] % R  # a b - c == 0 at row 1
    if n > 4:
        for t in tabs:
            t[2], t[3] = 0, R - 1
        tabs[1][4] = 0
    return tabs


def _want(expr, tabs):
    from quill_amd.field import fr_array
    n = len(tabs[0])
    vals = [expr.evaluate([t[x] for t in tabs]) for x in range(n)]
    return vals, fr_array(vals)


@pytest.fixture(scope="module")
def cases():
    """tables and expected words per (nvars, expression): built once, read only"""
    out = {}
    for nv in (0, 1, 9):
        tabs = _tables(nv, 900 + nv)
        out[nv] = (tabs, {k: _want(e, tabs) for k, e in _exprs().items()})
    return out


@pytest.mark.parametrize("nvars", [0, 1, 9])
def test_expr_column_matches_evaluate(dev, cases, nvars):
    """both entries, every expression; 2^9 rows are two blocks of the kernel"""
    from quill_amd import VirtualPolynomialStore, expr_column
    tabs, want = cases[nvars]
    hs, ds = VirtualPolynomialStore(nvars), VirtualPolynomialStore(nvars, dev)
    for t in tabs:
        hs.allocate_polynomial(t)
        ds.allocate_polynomial(t)
    for name, e in _exprs().items():
        vals, words = want[name]
        assert expr_column(hs, hs.new_virtual_from_expr(e), dev) == vals, name
        col = expr_column(ds, ds.new_virtual_from_expr(e))
        got = col.to_numpy()
        col.close()
        assert np.array_equal(got, words), name
    # the rows that are 0 mod r are zero words, not r
    assert want["a_plus_1"][0][0] == 0 and not want["a_plus_1"][1][0].any()
    if nvars:
        assert want["ab_minus_c"][0][1] == 0 and not want["ab_minus_c"][1][1].any()
    assert len(ds.polynomials) == 5


def test_expr_column_sharded(cases):
    """world 2: nvars is global, each rank passes and receives its block"""
    from quill_amd import VirtualPolynomialStore, expr_column
    tabs, want = cases[9]
    L = 1 << 8

    def fn(dev, rank, world):
        st = VirtualPolynomialStore(9, dev)
        for t in tabs:
            st.allocate_polynomial(t[rank * L:(rank + 1) * L])
        res = {}
        for name, e in _exprs().items():
            col = expr_column(st, st.new_virtual_from_expr(e))
            res[name] = col.to_numpy()
            col.close()
        return res

    for rank, res in enumerate(run_ranks(2, fn)):
        for name, got in res.items():
            assert np.array_equal(got, want[name][1][rank * L:(rank + 1) * L]), (rank, name)


def _sum_of_pairs(k):
    """k distinct degree-2 monomials over 17 tables"""
    from quill_amd import VirtualPolyExpr as E
    pairs = [(i, j) for i in range(17) for j in range(i + 1, 17)][:k]
    assert len(pairs) == k
    e = E.Input(pairs[0][0]) * E.Input(pairs[0][1])
    for i, j in pairs[1:]:
        e = e + E.Input(i) * E.Input(j)
    return e


def test_expr_column_statuses(dev):
    import quill_amd as q
    from quill_amd import VirtualPolyExpr as E, lib
    from quill_amd.field import fr_array
    from quill_amd.hyperplonk import _program_c
    L = lib()
    nv, n = 3, 8
    rnd = random.Random(3)
    host = [fr_array([rnd.randrange(R) for _ in range(n)]) for _ in range(17)]
    vecs = [q.DeviceVec(dev, n) for _ in host]
    for v, a in zip(vecs, host):
        assert L.qg_buf_upload(v.h, a.ctypes.data_as(U64P), n) == 0
    hp = (U64P * 17)(*[a.ctypes.data_as(U64P) for a in host])
    dp = (C.c_void_p * 17)(*[v.h.value for v in vecs])
    prog, plen, carr, nc = _program_c(E.Input(0) * E.Input(1) + E.Const(9))
    cp = carr.ctypes.data_as(U64P)
    out_h = np.zeros((n, 4), dtype=np.uint64)
    oh = out_h.ctypes.data_as(U64P)
    out_d = q.DeviceVec(dev, n)

    assert L.qg_expr_column(dev.h, nv, 17, hp, prog, plen, cp, nc, oh) == 0
    assert L.qg_expr_column_dev(dev.h, nv, 17, dp, prog, plen, cp, nc, out_d.h) == 0
    assert np.array_equal(out_d.to_numpy(), out_h)
    # nulls
    assert L.qg_expr_column(None, nv, 17, hp, prog, plen, cp, nc, oh) == -1
    assert L.qg_expr_column(dev.h, nv, 17, None, prog, plen, cp, nc, oh) == -1
    assert L.qg_expr_column(dev.h, nv, 17, hp, None, plen, cp, nc, oh) == -1
    assert L.qg_expr_column(dev.h, nv, 17, hp, prog, 0, cp, nc, oh) == -1
    assert L.qg_expr_column(dev.h, nv, 17, hp, prog, plen, None, nc, oh) == -1
    assert L.qg_expr_column(dev.h, nv, 17, hp, prog, plen, cp, nc, None) == -1
    hole = (U64P * 17)(*[a.ctypes.data_as(U64P) for a in host])
    hole[5] = None
    assert L.qg_expr_column(dev.h, nv, 17, hole, prog, plen, cp, nc, oh) == -1
    assert L.qg_expr_column_dev(None, nv, 17, dp, prog, plen, cp, nc, out_d.h) == -1
    assert L.qg_expr_column_dev(dev.h, nv, 17, None, prog, plen, cp, nc, out_d.h) == -1
    assert L.qg_expr_column_dev(dev.h, nv, 17, dp, None, plen, cp, nc, out_d.h) == -1
    assert L.qg_expr_column_dev(dev.h, nv, 17, dp, prog, plen, cp, nc, None) == -1
    dhole = (C.c_void_p * 17)(*[v.h.value for v in vecs])
    dhole[5] = None
    assert L.qg_expr_column_dev(dev.h, nv, 17, dhole, prog, plen, cp, nc, out_d.h) == -1
    # an input index outside the tables given
    assert L.qg_expr_column_dev(dev.h, nv, 1, dp, prog, plen, cp, nc, out_d.h) == -1
    # short buffers: the output, a table
    short = q.DeviceVec(dev, n - 1)
    assert L.qg_expr_column_dev(dev.h, nv, 17, dp, prog, plen, cp, nc, short.h) == -1
    dshort = (C.c_void_p * 17)(*[v.h.value for v in vecs])
    dshort[16] = short.h.value
    assert L.qg_expr_column_dev(dev.h, nv, 17, dshort, prog, plen, cp, nc, out_d.h) == -1
    # out aliases a table: the same buffer, an overlapping view, the host array
    assert L.qg_expr_column_dev(dev.h, nv, 17, dp, prog, plen, cp, nc, vecs[1].h) == -1
    big = q.DeviceVec(dev, 2 * n)
    view_t, view_o = big.view(0, n), big.view(n - 1, n)
    dview = (C.c_void_p * 17)(*[v.h.value for v in vecs])
    dview[16] = view_t.h.value
    assert L.qg_expr_column_dev(dev.h, nv, 17, dview, prog, plen, cp, nc, view_o.h) == -1
    assert L.qg_expr_column(dev.h, nv, 17, hp, prog, plen, cp, nc,
                            host[2].ctypes.data_as(U64P)) == -1
    # 128 monomials compile, 129 do not: QG_ERR_UNSUPPORTED, no interpreter fallback
    for k, rc in ((128, 0), (129, -4)):
        p2, l2, c2, n2 = _program_c(_sum_of_pairs(k))
        assert L.qg_expr_column_dev(dev.h, nv, 17, dp, p2, l2, c2.ctypes.data_as(U64P), n2,
                                    out_d.h) == rc
        assert L.qg_expr_column(dev.h, nv, 17, hp, p2, l2, c2.ctypes.data_as(U64P), n2, oh) == rc
    assert "monomials" in L.qg_last_error(dev.h).decode()
    for v in [view_t, view_o, big, short, out_d] + vecs:
        v.close()


# ---- a packed source column a + 256 b against a packed table column ----
def _packed_case():
    """source 2^6 rows of (a, b) with a, b < 16; table 2^8 rows j -> (j % 16) +
    256 (j // 16); the multiplicity column counted by hand"""
    rnd = random.Random(256)
    a = [rnd.randrange(16) for _ in range(1 << 6)]
    b = [rnd.randrange(16) for _ in range(1 << 6)]
    tab = [(j % 16) + 256 * (j // 16) for j in range(1 << 8)]
    first = {}
    for j, v in enumerate(tab):
        first.setdefault(v, j)
    mult = [0] * len(tab)
    for x, y in zip(a, b):
        mult[first[x + 256 * y]] += 1
    return a, b, tab, mult


def _packed_stores(dev, resident):
    from quill_amd import VirtualPolyExpr as E, VirtualPolynomialStore
    a, b, tab, _ = _packed_case()
    ss = VirtualPolynomialStore(6, dev if resident else None)
    ds = VirtualPolynomialStore(8, dev if resident else None)
    ss.allocate_polynomial(a)
    ss.allocate_polynomial(b)
    ds.allocate_polynomial(tab)
    sc = [ss.new_virtual_from_expr(E.Input(0) + E.Const(256) * E.Input(1))]
    dc = [ds.new_virtual_from_input(0)]
    return ss, ds, sc, dc


@pytest.mark.parametrize("resident", [False, True])
def test_lookup_multiplicities_materialise(dev, resident):
    from quill_amd.logup import lookup_multiplicities
    mult = _packed_case()[3]
    ss, ds, sc, dc = _packed_stores(dev, resident)
    with pytest.raises(ValueError, match="plain Input"):
        lookup_multiplicities(ss, sc, ds, dc, dev)
    m = lookup_multiplicities(ss, sc, ds, dc, dev, materialise=True)
    assert (m.to_list() if resident else m) == mult
    assert sum(mult) == 1 << 6
    # nothing was allocated into a store
    assert (len(ss.polynomials), len(ds.polynomials)) == (2, 1)
    assert (len(ss.virtual_polys), len(ds.virtual_polys)) == (1, 1)


@pytest.mark.parametrize("resident", [False, True])
def test_lookup_prove_over_expression_column(dev, resident):
    """LookupProof.prove(..., multiplicities=None) with the packed expression
    column equals o.lookup_prove given the hand-counted column; the stores hold
    what the oracle's hold; the proof verifies"""
    from quill_amd import KZG, EvaluationClaim, Transcript
    from quill_amd.logup import LookupProof
    a, b, tab, mult = _packed_case()
    ss, ds, sc, dc = _packed_stores(dev, resident)
    oss, ods = o.VirtualPolynomialStore(6), o.VirtualPolynomialStore(8)
    oss.allocate_polynomial(a)
    oss.allocate_polynomial(b)
    ods.allocate_polynomial(tab)
    ods.allocate_polynomial(mult)
    osc = [oss.new_virtual_from_expr(o.Expr.input(0) + o.Expr.const(256) * o.Expr.input(1))]
    odc = [ods.new_virtual_from_input(0)]
    om = ods.new_virtual_from_input(1)
    kzg, okzg = KZG.trusted_setup(1 << 8, TAU, dev), o.KZG(1 << 8, TAU)
    t, ot = Transcript(b"packed"), o.Transcript(b"packed")
    proof, (pl, pr) = LookupProof.prove(ss, sc, ds, dc, None, t, kzg)
    oproof, (opl, opr) = o.lookup_prove(oss, osc, ods, odc, om, ot, okzg)
    assert (pl, pr) == (opl, opr) and t.state == ot.state
    sp = proof.set_inclusion_proof
    assert sp.denom_left_commitment == oproof.denom_left_commitment
    assert sp.denom_right_commitment == oproof.denom_right_commitment
    for g, w in ((sp.sumcheck_proof_left, oproof.sumcheck_proof_left),
                 (sp.sumcheck_proof_right, oproof.sumcheck_proof_right)):
        assert (g.num_vars, g.claimed_sum, g.r_polys) == (w.num_vars, w.claimed_sum % R, w.r_polys)
    for g, w in ((sp.opening_proof_denom_left, oproof.opening_proof_denom_left),
                 (sp.opening_proof_denom_right, oproof.opening_proof_denom_right)):
        assert (g.evaluation_point, g.evaluation, g.s_comm) == (w.evaluation_point, w.evaluation,
                                                                w.s_comm)
        for k in ("poly_opening", "poly_opening_inv", "s_opening", "s_opening_inv"):
            assert (getattr(g, k).x, getattr(g, k).y, getattr(g, k).proof) == tuple(getattr(w, k))
    for st, ost in ((ss, oss), (ds, ods)):
        polys = [p.to_list() for p in st.polynomials] if resident else st.polynomials
        assert polys == ost.polynomials and len(st.virtual_polys) == len(ost.virtual_polys)
    packed = [x + 256 * y for x, y in zip(a, b)]
    vt = Transcript(b"packed")
    proof.verify(vt, kzg, [EvaluationClaim(pl, o.mle_evaluate(packed, pl))],
                 [EvaluationClaim(pr, o.mle_evaluate(tab, pr))],
                 EvaluationClaim(pr, o.mle_evaluate(mult, pr)))
    ovt = o.Transcript(b"packed")
    o.lookup_verify(oproof, ovt, okzg, [(pl, o.mle_evaluate(packed, pl))],
                    [(pr, o.mle_evaluate(tab, pr))], (pr, o.mle_evaluate(mult, pr)))
    assert vt.state == ovt.state
    kzg.close()
