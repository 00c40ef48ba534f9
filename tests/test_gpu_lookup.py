"""Lookup multiplicities on the device (qg_lookup_multiplicities[_dev],
csrc/lookup.hip) and LookupProof.prove(..., multiplicities=None).

The expected column is a dict count written here: m[j] = number of source rows
equal to table row j, a tuple the table holds at several rows counted at the
lowest of them.  Columns are raw (n, 4) uint64 Montgomery arrays, so the same
words go through the host entry and (uploaded) through the _dev entry."""
import ctypes as C
import random

import numpy as np
import pytest

import quill_oracle as o

pytestmark = pytest.mark.gpu
R = o.R_MOD
TAU = 0x1234567890ABCDEF1122334455667788
U64P = C.POINTER(C.c_uint64)
LDS_ROWS = 16384  # csrc/lookup.hip LK_LDS_ROWS: per-block LDS counters up to here


def _mont(vals):
    """ints -> (n, 4) uint64 Montgomery words (converted once per distinct value)"""
    from quill_amd.field import fr_array
    vals = [int(v) for v in vals]
    uniq = sorted(set(vals))
    pos = {v: i for i, v in enumerate(uniq)}
    return np.ascontiguousarray(fr_array(uniq)[[pos[v] for v in vals]])


def _keys(cols):
    a = np.ascontiguousarray(np.concatenate(cols, axis=1))
    return [r.tobytes() for r in a]


def _expected(src, tab):
    """(m as ints, lowest source row in no table row or -1)"""
    first = {}
    for j, k in enumerate(_keys(tab)):
        first.setdefault(k, j)
    m = [0] * tab[0].shape[0]
    miss = -1
    for i, k in enumerate(_keys(src)):
        j = first.get(k)
        if j is None:
            miss = i if miss < 0 else miss
        else:
            m[j] += 1
    return m, miss


def _ptrs(arrs):
    return (U64P * max(len(arrs), 1))(*[a.ctypes.data_as(U64P) for a in arrs])


def _host(dev, src, tab, ns=None, nt=None, ncols=None, out=None):
    from quill_amd import lib
    ns = src[0].shape[0] if ns is None else ns
    nt = tab[0].shape[0] if nt is None else nt
    out = np.zeros((max(nt, 1), 4), dtype=np.uint64) if out is None else out
    miss = C.c_int64(-7)
    rc = lib().qg_lookup_multiplicities(dev.h, len(src) if ncols is None else ncols, _ptrs(src),
                                        ns, _ptrs(tab), nt, out.ctypes.data_as(U64P),
                                        C.byref(miss))
    return rc, out[:nt], miss.value


def _upload(dev, a):
    from quill_amd import DeviceVec, lib
    from quill_amd._lib import check
    v = DeviceVec(dev, a.shape[0])
    check(lib().qg_buf_upload(v.h, a.ctypes.data_as(U64P), a.shape[0]), dev.h)
    return v


def _dev(dev, src, tab, ns=None, nt=None, ncols=None, out=None):
    """src / tab: DeviceVec lists"""
    from quill_amd import DeviceVec, lib
    ns = src[0].n if ns is None else ns
    nt = tab[0].n if nt is None else nt
    o_ = DeviceVec(dev, max(nt, 1)) if out is None else out
    miss = C.c_int64(-7)
    sp = (C.c_void_p * max(len(src), 1))(*[v.h.value for v in src])
    tp = (C.c_void_p * max(len(tab), 1))(*[v.h.value for v in tab])
    rc = lib().qg_lookup_multiplicities_dev(dev.h, len(src) if ncols is None else ncols, sp, ns,
                                            tp, nt, o_.h, C.byref(miss))
    res = o_.to_numpy(nt) if rc == 0 else None
    if out is None:
        o_.close()
    return rc, res, miss.value


def _last_error(dev):
    from quill_amd import lib
    return lib().qg_last_error(dev.h).decode()


def _check(dev, src, tab):
    """both entries against the dict count; returns the column (raw words)"""
    m, miss = _expected(src, tab)
    assert miss == -1
    want = _mont(m)
    rc, got, fm = _host(dev, src, tab)
    assert (rc, fm) == (0, -1), _last_error(dev)
    assert np.array_equal(got, want)
    ds, dt = [_upload(dev, a) for a in src], [_upload(dev, a) for a in tab]
    rc, gotd, fm = _dev(dev, ds, dt)
    for v in ds + dt:
        v.close()
    assert (rc, fm) == (0, -1), _last_error(dev)
    assert np.array_equal(gotd, want)
    assert sum(m) == src[0].shape[0]
    return got


def _pick(tab, idx):
    return [np.ascontiguousarray(t[idx]) for t in tab]


def test_single_row(dev):
    _check(dev, [_mont([5])], [_mont([5])])


def test_xor42_byte_table(dev):
    rnd = random.Random(42)
    by = [rnd.randrange(256) for _ in range(1 << 6)]
    _check(dev, [_mont(by), _mont([b ^ 42 for b in by])],
           [_mont(range(256)), _mont([i ^ 42 for i in range(256)])])


def test_rows_differing_in_one_limb(dev):
    """column 0 agrees on every table row; column 1 differs from a base word in
    exactly one 32-bit word (both halves of each of the four 64-bit limbs), plus
    the words of 0, 1 and r - 1; every row is hit a different number of times"""
    base = np.array([0x1111111111111111, 0x2222222222222222, 0x3333333333333333,
                     0x0444444444444444], dtype=np.uint64)  # top limb below r's: canonical
    words = [base.copy()]
    for limb in range(4):
        for bit in (0, 32):
            w = base.copy()
            w[limb] ^= np.uint64(1 << bit)
            words.append(w)
    col1 = np.ascontiguousarray(np.concatenate([np.stack(words), _mont([0, 1, R - 1])]))
    nt = col1.shape[0]
    assert len({r.tobytes() for r in col1}) == nt == 12
    tab = [_mont([7] * nt), col1]
    idx = [j for j in range(nt) for _ in range(j + 1)]
    random.Random(3).shuffle(idx)
    got = _check(dev, _pick(tab, idx), tab)
    assert np.array_equal(got, _mont(range(1, nt + 1)))


def test_duplicate_table_rows(dev):
    """adjacent and far-apart duplicates, row 0 repeated at the last row: the
    lowest index takes the whole count, and two calls agree"""
    nt = 300
    a = list(range(nt))
    a[11] = a[10]        # adjacent
    a[200] = a[37]       # far apart
    a[250] = a[37]       # a third copy
    a[nt - 1] = a[0]     # row 0 again at the last row
    tab = [_mont(a), _mont([x * x % 97 for x in a])]
    rnd = random.Random(9)
    idx = [rnd.randrange(nt) for _ in range(2000)] + [0, nt - 1, 10, 11, 37, 200, 250]
    src = _pick(tab, idx)
    got = _check(dev, src, tab)
    m, _ = _expected(src, tab)
    assert m[11] == m[200] == m[250] == m[nt - 1] == 0
    assert m[0] > 0 and m[10] > 0 and m[37] > 0
    assert np.array_equal(_check(dev, src, tab), got)


def _three_col_table(nt):
    j = np.arange(nt)
    return [_mont(j % 7), _mont(j // 7), _mont((j * j) % 5)]


def test_non_power_of_two_lengths(dev):
    tab = _three_col_table(257)
    rnd = random.Random(257)
    _check(dev, _pick(tab, [rnd.randrange(257) for _ in range(1000)]), tab)


def _skewed(nt, ns, seed):
    """half of the source rows hit one table row, the rest are uniform"""
    rnd = np.random.RandomState(seed)
    idx = rnd.randint(0, nt, size=ns)
    idx[rnd.rand(ns) < 0.5] = nt // 3
    return idx


@pytest.mark.parametrize("blocks", [None, "3"])
def test_many_blocks_skewed(dev, monkeypatch, blocks):
    """2^12 table rows, 2^16 source rows, 3 columns: 64 count blocks; capped
    to 3 blocks every thread runs 22 grid-stride rounds, the last one ragged"""
    if blocks:
        monkeypatch.setenv("QG_LOOKUP_BLOCKS", blocks)
    tab = _three_col_table(1 << 12)
    _check(dev, _pick(tab, _skewed(1 << 12, 1 << 16, 1)), tab)


@pytest.mark.parametrize("nt", [LDS_ROWS, LDS_ROWS + 1])
@pytest.mark.parametrize("blocks", [None, "2"])
def test_lds_counter_threshold(dev, monkeypatch, nt, blocks):
    """the largest table counted in LDS and the smallest counted with merged
    global atomics, skewed and uniform hits, with and without grid-stride rounds"""
    if blocks:
        monkeypatch.setenv("QG_LOOKUP_BLOCKS", blocks)
    tab = _three_col_table(nt)
    ns = (1 << 15) + 77
    idx = _skewed(nt, ns, nt)
    idx[:4] = [0, nt - 1, nt - 1, LDS_ROWS - 1]  # the edge rows are hit
    _check(dev, _pick(tab, idx), tab)


@pytest.mark.parametrize("bits", ["0", "3"])
def test_forced_collisions(dev, monkeypatch, bits):
    """QG_LOOKUP_HASH_BITS = 0: every row in one probe chain; 3: eight chains"""
    a = list(range(256))
    a[1], a[128], a[255] = a[0], a[5], a[0]
    tab = [_mont(a), _mont([x ^ 42 for x in a])]
    rnd = random.Random(10)
    src = _pick(tab, [rnd.randrange(256) for _ in range(1 << 10)])
    free = _check(dev, src, tab)
    monkeypatch.setenv("QG_LOOKUP_HASH_BITS", bits)
    assert np.array_equal(_check(dev, src, tab), free)


def test_missing_rows(dev):
    """two absent source rows (one equal to a table row in column 0 only):
    QG_ERR_ASSERT, the lower index, named in the error; nothing of the failed
    call survives into the next one"""
    tab = [_mont(range(256)), _mont([i ^ 42 for i in range(256)])]
    rnd = random.Random(4)
    by = [rnd.randrange(256) for _ in range(500)]
    s1, s2 = list(by), [b ^ 42 for b in by]
    s2[333] = s2[333] ^ 1          # column 0 still matches table row by[333]
    s1[401], s2[401] = 1000, 1001  # in neither column
    src = [_mont(s1), _mont(s2)]
    assert _expected(src, tab)[1] == 333
    rc, _, fm = _host(dev, src, tab)
    assert (rc, fm) == (-5, 333)
    assert "333" in _last_error(dev)
    ds, dt = [_upload(dev, a) for a in src], [_upload(dev, a) for a in tab]
    rc, _, fm = _dev(dev, ds, dt)
    assert (rc, fm) == (-5, 333)
    assert "333" in _last_error(dev)
    # first_missing is optional
    from quill_amd import lib
    out = np.zeros((256, 4), dtype=np.uint64)
    assert lib().qg_lookup_multiplicities(dev.h, 2, _ptrs(src), 500, _ptrs(tab), 256,
                                          out.ctypes.data_as(U64P), None) == -5
    for v in ds + dt:
        v.close()
    _check(dev, [_mont(by), _mont([b ^ 42 for b in by])], tab)


def test_scratch_reuse(dev):
    """a large call, a small one, the large one again on one context"""
    big = _three_col_table(5000)
    bsrc = _pick(big, _skewed(5000, 20000, 2))
    small = [_mont([3, 4, 3])]
    ssrc = [_mont([4, 4, 3, 3, 3])]
    first = _check(dev, bsrc, big)
    assert np.array_equal(_check(dev, ssrc, small), _mont([3, 2, 0]))
    assert np.array_equal(_check(dev, bsrc, big), first)


def test_argument_errors(dev):
    import quill_amd as q
    from quill_amd import lib
    col = _mont(range(8))
    src, tab = [col.copy()], [col.copy()]
    assert _host(dev, src, tab, ns=0)[0] == -1
    assert _host(dev, src, tab, nt=0)[0] == -1
    assert _host(dev, src, tab, ncols=0)[0] == -1
    many = [col.copy() for _ in range(17)]
    assert _host(dev, many, many)[0] == -4
    assert _host(dev, many[:16], many[:16])[0] == 0
    assert _host(dev, src, tab, out=tab[0])[0] == -1  # out_m aliases a column
    assert lib().qg_lookup_multiplicities(dev.h, 1, None, 8, _ptrs(tab), 8,
                                          col.ctypes.data_as(U64P), None) == -1
    assert lib().qg_lookup_multiplicities(None, 1, _ptrs(src), 8, _ptrs(tab), 8,
                                          col.ctypes.data_as(U64P), None) == -1
    ds, dt = [_upload(dev, col)], [_upload(dev, col)]
    assert _dev(dev, ds, dt, ns=0)[0] == -1
    assert _dev(dev, ds, dt, nt=0)[0] == -1
    assert _dev(dev, ds, dt, ncols=0)[0] == -1
    assert _dev(dev, ds * 17, dt * 17)[0] == -4
    assert _dev(dev, ds, dt, ns=9)[0] == -1   # a buffer shorter than its stated length
    assert _dev(dev, ds, dt, nt=9)[0] == -1
    short = q.DeviceVec(dev, 7)
    assert _dev(dev, ds, dt, out=short)[0] == -1
    assert _dev(dev, ds, dt, out=dt[0])[0] == -1  # out_m aliases a column
    assert _dev(dev, ds, dt, out=ds[0])[0] == -1
    view = dt[0].view(2, 6)                       # ... or overlaps one
    assert _dev(dev, ds, [view], nt=6, out=dt[0])[0] == -1
    view.close()
    assert _dev(dev, ds, dt)[0] == 0
    # over the caps: statuses, not launches (no such buffers exist)
    assert _dev(dev, ds, dt, nt=1 << 31, out=short)[0] == -4
    assert _dev(dev, ds, dt, ns=1 << 32, out=short)[0] == -4
    # a context with a two-rank loopback communicator attached
    group = q.Device.loopback_group(2)
    d2 = q.Device(0)
    d2.attach_loopback(group, 0)
    assert d2.comm_info()["sharded"]
    assert _host(d2, src, tab)[0] == -4
    assert "sharded" in _last_error(d2)
    d2.close()
    lib().qg_loopback_destroy(group)
    for v in ds + dt + [short]:
        v.close()


def _xor_case(ns, resident, dev, bad_row=None):
    from quill_amd import VirtualPolynomialStore
    rnd = random.Random(42)
    c1, c2 = list(range(256)), [i ^ 42 for i in range(256)]
    by = [rnd.randrange(256) for _ in range(1 << ns)]
    s1, s2 = list(by), [b ^ 42 for b in by]
    if bad_row is not None:
        s2[bad_row] ^= 1
    mult = [0] * 256
    for b in by:
        mult[b] += 1
    ss = VirtualPolynomialStore(ns, dev if resident else None)
    ds = VirtualPolynomialStore(8, dev if resident else None)
    oss, ods = o.VirtualPolynomialStore(ns), o.VirtualPolynomialStore(8)
    for tb in (s1, s2):
        ss.allocate_polynomial(tb)
        oss.allocate_polynomial(tb)
    for tb in (c1, c2):
        ds.allocate_polynomial(tb)
        ods.allocate_polynomial(tb)
    ods.allocate_polynomial(mult)
    return (s1, s2, c1, c2, mult), (ss, ds), (oss, ods)


@pytest.mark.parametrize("resident", [False, True])
def test_lookup_prove_counts_multiplicities(dev, resident):
    """LookupProof.prove(..., multiplicities=None) at the XOR-42 shape: proof,
    points, stores and transcript equal o.lookup_prove given the hand-counted
    column, and LookupProof.verify accepts it"""
    from quill_amd import KZG, EvaluationClaim, Transcript
    from quill_amd.logup import LookupProof, lookup_multiplicities
    (s1, s2, c1, c2, mult), (ss, ds), (oss, ods) = _xor_case(6, resident, dev)
    sc = [ss.new_virtual_from_input(0), ss.new_virtual_from_input(1)]
    dc = [ds.new_virtual_from_input(0), ds.new_virtual_from_input(1)]
    osc = [oss.new_virtual_from_input(0), oss.new_virtual_from_input(1)]
    odc = [ods.new_virtual_from_input(0), ods.new_virtual_from_input(1)]
    om = ods.new_virtual_from_input(2)
    m = lookup_multiplicities(ss, sc, ds, dc, dev)
    assert (m.to_list() if resident else m) == mult
    kzg, okzg = KZG.trusted_setup(1 << 8, TAU, dev), o.KZG(1 << 8, TAU)
    t, ot = Transcript(b"lookup"), o.Transcript(b"lookup")
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
    polys = [p.to_list() for p in ds.polynomials] if resident else ds.polynomials
    assert polys == ods.polynomials and len(ds.virtual_polys) == len(ods.virtual_polys)
    vt = Transcript(b"lookup")
    proof.verify(vt, kzg,
                 [EvaluationClaim(pl, o.mle_evaluate(s1, pl)),
                  EvaluationClaim(pl, o.mle_evaluate(s2, pl))],
                 [EvaluationClaim(pr, o.mle_evaluate(c1, pr)),
                  EvaluationClaim(pr, o.mle_evaluate(c2, pr))],
                 EvaluationClaim(pr, o.mle_evaluate(mult, pr)))
    ovt = o.Transcript(b"lookup")
    o.lookup_verify(oproof, ovt, okzg,
                    [(pl, o.mle_evaluate(s1, pl)), (pl, o.mle_evaluate(s2, pl))],
                    [(pr, o.mle_evaluate(c1, pr)), (pr, o.mle_evaluate(c2, pr))],
                    (pr, o.mle_evaluate(mult, pr)))
    assert vt.state == ovt.state


@pytest.mark.parametrize("resident", [False, True])
def test_lookup_prove_rejects_row_outside_table(dev, resident):
    """the count fails before the prover touches the transcript"""
    from quill_amd import KZG, QuillGpuError, Transcript
    from quill_amd.logup import LookupProof
    _, (ss, ds), _ = _xor_case(6, resident, dev, bad_row=19)
    sc = [ss.new_virtual_from_input(0), ss.new_virtual_from_input(1)]
    dc = [ds.new_virtual_from_input(0), ds.new_virtual_from_input(1)]
    kzg = KZG.trusted_setup(1 << 8, TAU, dev)
    t = Transcript(b"lookup")
    before = bytes(t.state)
    with pytest.raises(QuillGpuError) as ei:
        LookupProof.prove(ss, sc, ds, dc, None, t, kzg)
    assert ei.value.code == -5 and "19" in str(ei.value)
    assert bytes(t.state) == before
    assert len(ds.polynomials) == 2 and len(ds.virtual_polys) == 2


def test_lookup_multiplicities_needs_input_columns(dev):
    from quill_amd import VirtualPolyExpr as E, VirtualPolynomialStore
    from quill_amd.logup import lookup_multiplicities
    ss, ds = VirtualPolynomialStore(1), VirtualPolynomialStore(1)
    ss.allocate_polynomial([1, 2])
    ds.allocate_polynomial([1, 2])
    bad = ss.new_virtual_from_expr(E.Input(0) + E.Const(1))
    good = ds.new_virtual_from_input(0)
    with pytest.raises(ValueError, match="plain Input"):
        lookup_multiplicities(ss, [bad], ds, [good], dev)
    assert lookup_multiplicities(ss, [ss.new_virtual_from_input(0)], ds, [good], dev) == [1, 1]
