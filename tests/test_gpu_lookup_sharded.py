"""Lookup multiplicities on sharded contexts (qg_lookup_multiplicities_dev with a
communicator attached, csrc/lookup.hip lookup_run_sharded) and
LookupProof.prove(..., multiplicities=None) on sharded device stores.

Ranks run as threads on one GPU over the in-process loopback communicator.
Rank r holds rows [r L, (r + 1) L) of every column; the expected column is a
dict count over the concatenated blocks, written here: m[j] = number of global
source rows equal to global table row j, a tuple the table holds at several
rows counted at the lowest of them.  Columns are raw (n, 4) uint64 Montgomery
arrays."""
import ctypes as C
import os
import random
import threading

import numpy as np
import pytest

import quill_oracle as o

pytestmark = pytest.mark.gpu
R = o.R_MOD
TAU = 0x1234567890ABCDEF1122334455667788
U64P = C.POINTER(C.c_uint64)
LDS_ROWS = 16384  # csrc/lookup.hip LK_LDS_ROWS: per-block LDS counters up to here


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
    """(global m as ints, lowest global source row in no table row or -1)"""
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


def _upload(dev, a):
    from quill_amd import DeviceVec, lib
    from quill_amd._lib import check
    v = DeviceVec(dev, a.shape[0])
    check(lib().qg_buf_upload(v.h, a.ctypes.data_as(U64P), a.shape[0]), dev.h)
    return v


def _block(cols, rank, world):
    n = cols[0].shape[0] // world
    return [np.ascontiguousarray(c[rank * n:(rank + 1) * n]) for c in cols]


def _call(dev, src, tab, ns=None, nt=None, out=None):
    """src / tab: DeviceVec lists -> (rc, block words or None, first_missing)"""
    from quill_amd import DeviceVec, lib
    ns = src[0].n if ns is None else ns
    nt = tab[0].n if nt is None else nt
    o_ = DeviceVec(dev, max(tab[0].n, 1)) if out is None else out
    miss = C.c_int64(-7)
    sp = (C.c_void_p * len(src))(*[v.h.value for v in src])
    tp = (C.c_void_p * len(tab))(*[v.h.value for v in tab])
    rc = lib().qg_lookup_multiplicities_dev(dev.h, len(src), sp, ns, tp, nt, o_.h, C.byref(miss))
    res = o_.to_numpy(nt) if rc == 0 else None
    if out is None:
        o_.close()
    return rc, res, miss.value


def _last_error(dev):
    from quill_amd import lib
    return lib().qg_last_error(dev.h).decode()


def _run(world, src, tab):
    """one sharded call on global columns -> per rank (rc, block, first_missing,
    collectives issued)"""
    def fn(dev, rank, world):
        ds = [_upload(dev, a) for a in _block(src, rank, world)]
        dt = [_upload(dev, a) for a in _block(tab, rank, world)]
        before = dev.counter("lookup_collectives")
        rc, got, fm = _call(dev, ds, dt)
        used = dev.counter("lookup_collectives") - before
        for v in ds + dt:
            v.close()
        return rc, got, fm, used
    return run_ranks(world, fn)


def _check(world, src, tab):
    """every rank's block against the slice of the dict count; returns m"""
    m, miss = _expected(src, tab)
    assert miss == -1 and sum(m) == src[0].shape[0]
    want = _mont(m)
    L = len(m) // world
    for rank, (rc, got, fm, used) in enumerate(_run(world, src, tab)):
        assert (rc, fm) == (0, -1)
        assert np.array_equal(got, want[rank * L:(rank + 1) * L]), rank
        assert 0 < used <= len(src) + 3
    return m


def _table(nt, ncols):
    """nt distinct rows of ncols columns"""
    j = np.arange(nt)
    if ncols == 1:
        return [_mont(j)]
    return [_mont(j % 7), _mont(j // 7), _mont((j * j) % 5)][:ncols]


def _pick(tab, idx):
    return [np.ascontiguousarray(t[idx]) for t in tab]


@pytest.mark.parametrize("ncols", [1, 3])
@pytest.mark.parametrize("world", [2, 4, 8])
def test_blocks_equal_global_count(world, ncols):
    """global table of 64 rows (8 per rank at world 8), 100 source rows per rank"""
    tab = _table(64, ncols)
    rnd = random.Random(world * 10 + ncols)
    idx = [rnd.randrange(64) for _ in range(100 * world)]
    m = _check(world, _pick(tab, idx), tab)
    assert max(m) > 1


def test_one_table_row_per_rank():
    tab = _table(8, 3)
    rnd = random.Random(8)
    _check(8, _pick(tab, [rnd.randrange(8) for _ in range(8 * 33)]), tab)


@pytest.mark.parametrize("nt", [LDS_ROWS, 1 << 15])
def test_lds_limit_is_the_global_length(nt):
    """16384 global rows: the largest table counted in LDS; 2^15: merged global
    atomics (each rank's block alone would fit the LDS counters).  2^12 source
    rows per rank, half of them on one table row."""
    world = 4
    tab = _table(nt, 2)
    rnd = np.random.RandomState(nt)
    ns = world << 12
    idx = rnd.randint(0, nt, size=ns)
    idx[rnd.rand(ns) < 0.5] = nt // 3
    idx[:4] = [0, nt - 1, nt - 1, LDS_ROWS - 1]  # the edge rows are hit
    _check(world, _pick(tab, idx), tab)


def test_counts_travel_to_the_owning_rank():
    """rank r's source rows all lie in rank (r + 1) mod W's table block: without
    the exchange every block would be zero"""
    world, L, S = 4, 16, 50
    tab = _table(world * L, 3)
    rnd = random.Random(77)
    idx = []
    for r in range(world):
        nxt = (r + 1) % world
        idx += [nxt * L + rnd.randrange(L) for _ in range(S)]
    m = _check(world, _pick(tab, idx), tab)
    assert all(sum(m[r * L:(r + 1) * L]) == S for r in range(world))


def test_duplicate_rows_across_ranks():
    """a tuple at global rows 3 (rank 0) and 10 (rank 1) is counted at row 3;
    one at rows 12 and 14 (both rank 1) at row 12"""
    a = list(range(16))
    a[10] = a[3]
    a[14] = a[12]
    tab = [_mont(a), _mont([x * x % 97 for x in a])]
    idx = [3, 10, 10, 12, 14, 14, 14, 0, 15, 10] + [10, 3, 14, 12, 7, 7, 3, 10, 14, 1]
    m = _check(2, _pick(tab, idx), tab)
    assert m[10] == m[14] == 0
    assert m[3] == idx.count(3) + idx.count(10) and m[12] == idx.count(12) + idx.count(14)


def test_one_probe_chain(monkeypatch):
    """QG_LOOKUP_HASH_BITS=0: every row of the gathered table in one probe chain"""
    tab = _table(64, 3)
    rnd = random.Random(5)
    src = _pick(tab, [rnd.randrange(64) for _ in range(400)])
    free = _check(4, src, tab)
    monkeypatch.setenv("QG_LOOKUP_HASH_BITS", "0")
    assert _check(4, src, tab) == free


def test_missing_rows_then_a_good_call():
    """a row missing on rank 1 only; rows missing on ranks 1 and 3 (the lower
    global row wins); every rank returns QG_ERR_ASSERT with the same global row,
    named in its error; a good call on the same contexts is right afterwards"""
    world, S = 4, 40
    tab = [_mont(range(64)), _mont([i ^ 42 for i in range(64)])]
    rnd = random.Random(4)
    by = [rnd.randrange(64) for _ in range(world * S)]
    good = [_mont(by), _mont([b ^ 42 for b in by])]
    s2 = [b ^ 42 for b in by]
    s2[1 * S + 17] ^= 1                    # column 0 still matches a table row
    one = [_mont(by), _mont(s2)]
    s1 = list(by)
    s1[3 * S + 2] = 1000                   # in no column of the table
    s2b = list(s2)
    s2b[1 * S + 17] = by[1 * S + 17] ^ 42  # rank 1's first bad row is now row 30
    s2b[1 * S + 30] ^= 1
    two = [_mont(s1), _mont(s2b)]
    assert _expected(one, tab)[1] == S + 17 and _expected(two, tab)[1] == S + 30
    want = _mont(_expected(good, tab)[0])
    L = 64 // world

    def fn(dev, rank, world):
        dt = [_upload(dev, a) for a in _block(tab, rank, world)]
        res = []
        for src in (one, two, good):
            ds = [_upload(dev, a) for a in _block(src, rank, world)]
            rc, got, fm = _call(dev, ds, dt)
            res.append((rc, got, fm, _last_error(dev) if rc else ""))
            for v in ds:
                v.close()
        for v in dt:
            v.close()
        return res

    for rank, res in enumerate(run_ranks(world, fn)):
        assert res[0][0] == -5 and res[0][2] == S + 17 and str(S + 17) in res[0][3]
        assert res[1][0] == -5 and res[1][2] == S + 30 and str(S + 30) in res[1][3]
        assert (res[2][0], res[2][2]) == (0, -1)
        assert np.array_equal(res[2][1], want[rank * L:(rank + 1) * L])


@pytest.mark.parametrize("how", ["tab_len", "short_out"])
def test_ranks_that_disagree_all_return_invalid(how):
    """rank 1 passes another tab_len, or an output buffer shorter than its block:
    every rank returns QG_ERR_INVALID and none waits in a collective; the next
    call on the same contexts is right"""
    import quill_amd as q
    world, L = 4, 16
    tab = _table(world * L, 2)
    rnd = random.Random(31)
    src = _pick(tab, [rnd.randrange(world * L) for _ in range(world * 20)])
    want = _mont(_expected(src, tab)[0])

    def fn(dev, rank, world):
        ds = [_upload(dev, a) for a in _block(src, rank, world)]
        dt = [_upload(dev, a) for a in _block(tab, rank, world)]
        if how == "tab_len":
            rc = _call(dev, ds, dt, nt=L - 1 if rank == 1 else L)[0]
        else:
            short = q.DeviceVec(dev, L - 1)
            rc = _call(dev, ds, dt, out=short if rank == 1 else None)[0]
            short.close()
        rc2, got, fm = _call(dev, ds, dt)
        for v in ds + dt:
            v.close()
        return rc, rc2, got, fm

    for rank, (rc, rc2, got, fm) in enumerate(run_ranks(world, fn)):
        assert rc == -1
        assert (rc2, fm) == (0, -1)
        assert np.array_equal(got, want[rank * L:(rank + 1) * L])


def test_global_caps():
    """W x tab_len = 2^31 or W x src_len = 2^32: QG_ERR_UNSUPPORTED on every rank
    after the header exchange alone (no such buffers exist: nothing is launched)"""
    col = _mont(range(8))

    def fn(dev, rank, world):
        ds, dt = [_upload(dev, col)], [_upload(dev, col)]
        before = dev.counter("lookup_collectives")
        a = _call(dev, ds, dt, nt=1 << 30)[0]
        b = _call(dev, ds, dt, ns=1 << 31)[0]
        used = dev.counter("lookup_collectives") - before
        c = _call(dev, ds, dt)[0]
        for v in ds + dt:
            v.close()
        return a, b, used, c

    for a, b, used, c in run_ranks(2, fn):
        assert (a, b, used, c) == (-4, -4, 2, 0)


def test_forced_one_rank_rccl_matches_plain_context(dev):
    """QG_FORCE_RCCL=1: a world-1 context with a real one-rank RCCL communicator
    goes through the sharded flow (ncclAllGather, grouped send/recv)"""
    import quill_amd as q
    old = os.environ.get("QG_FORCE_RCCL")
    os.environ["QG_FORCE_RCCL"] = "1"
    try:
        rdev = q.Device(0)
        rdev.attach_comm(0, 1, q.Device.comm_unique_id())
    finally:
        if old is None:
            os.environ.pop("QG_FORCE_RCCL")
        else:
            os.environ["QG_FORCE_RCCL"] = old
    assert rdev.comm_info()["kind"] == "rccl" and rdev.comm_info()["sharded"]
    tab = _table(300, 3)
    rnd = random.Random(300)
    src = _pick(tab, [rnd.randrange(300) for _ in range(2000)])
    res = []
    for d in (dev, rdev):
        ds, dt = [_upload(d, a) for a in src], [_upload(d, a) for a in tab]
        before = d.counter("lookup_collectives")
        rc, got, fm = _call(d, ds, dt)
        res.append((rc, got, fm, d.counter("lookup_collectives") - before))
        for v in ds + dt:
            v.close()
    rdev.close()
    assert (res[0][0], res[0][2], res[0][3]) == (0, -1, 0)
    assert (res[1][0], res[1][2], res[1][3]) == (0, -1, 3 + 3)
    assert np.array_equal(res[0][1], res[1][1])
    assert np.array_equal(res[0][1], _mont(_expected(src, tab)[0]))


# ---- LookupProof.prove(..., multiplicities=None) on sharded device stores ----
def _xor_lists(bad_row=None):
    """the XOR-42 shape: source 2^6 rows, table 2^8 rows"""
    rnd = random.Random(42)
    c1, c2 = list(range(256)), [i ^ 42 for i in range(256)]
    by = [rnd.randrange(256) for _ in range(1 << 6)]
    s1, s2 = list(by), [b ^ 42 for b in by]
    if bad_row is not None:
        s2[bad_row] ^= 1
    mult = [0] * 256
    for b in by:
        mult[b] += 1
    return s1, s2, c1, c2, mult


@pytest.fixture(scope="module")
def xor_oracle():
    """o.lookup_prove given the hand-counted column: computed once, read only"""
    s1, s2, c1, c2, mult = _xor_lists()
    oss, ods = o.VirtualPolynomialStore(6), o.VirtualPolynomialStore(8)
    for tb in (s1, s2):
        oss.allocate_polynomial(tb)
    for tb in (c1, c2, mult):
        ods.allocate_polynomial(tb)
    osc = [oss.new_virtual_from_input(0), oss.new_virtual_from_input(1)]
    odc = [ods.new_virtual_from_input(0), ods.new_virtual_from_input(1)]
    om = ods.new_virtual_from_input(2)
    okzg = o.KZG(1 << 8, TAU)
    ot = o.Transcript(b"lookup")
    oproof, pts = o.lookup_prove(oss, osc, ods, odc, om, ot, okzg)
    return oproof, pts, bytes(ot.state), okzg, ods


def _sharded_stores(dev, rank, world, lists):
    from quill_amd import VirtualPolynomialStore
    s1, s2, c1, c2, _ = lists
    ss, ds = VirtualPolynomialStore(6, dev), VirtualPolynomialStore(8, dev)
    for tb in (s1, s2):
        L = len(tb) // world
        ss.allocate_polynomial(tb[rank * L:(rank + 1) * L])
    for tb in (c1, c2):
        L = len(tb) // world
        ds.allocate_polynomial(tb[rank * L:(rank + 1) * L])
    sc = [ss.new_virtual_from_input(0), ss.new_virtual_from_input(1)]
    dc = [ds.new_virtual_from_input(0), ds.new_virtual_from_input(1)]
    return ss, ds, sc, dc


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_lookup_prove_counts_multiplicities(world, xor_oracle):
    """every rank's proof, points and transcript state equal o.lookup_prove given
    the hand-counted column; both verifiers accept; each rank's store blocks are
    the slices of the oracle's tables"""
    from quill_amd import KZG, EvaluationClaim, Transcript
    from quill_amd.logup import LookupProof
    oproof, (opl, opr), ostate, okzg, ods = xor_oracle
    lists = _xor_lists()
    s1, s2, c1, c2, mult = lists

    def fn(dev, rank, world):
        ss, ds, sc, dc = _sharded_stores(dev, rank, world, lists)
        kzg = KZG.trusted_setup(1 << 8, TAU, dev)
        t = Transcript(b"lookup")
        proof, pts = LookupProof.prove(ss, sc, ds, dc, None, t, kzg)
        polys = [p.to_list() for p in ds.polynomials]
        nvirt = len(ds.virtual_polys)
        kzg.close()
        return proof, pts, bytes(t.state), polys, nvirt

    outs = run_ranks(world, fn)
    L = 256 // world
    for rank, (proof, (pl, pr), state, polys, nvirt) in enumerate(outs):
        assert (pl, pr) == (opl, opr) and state == ostate
        sp = proof.set_inclusion_proof
        assert sp.denom_left_commitment == oproof.denom_left_commitment
        assert sp.denom_right_commitment == oproof.denom_right_commitment
        for g, w in ((sp.sumcheck_proof_left, oproof.sumcheck_proof_left),
                     (sp.sumcheck_proof_right, oproof.sumcheck_proof_right)):
            assert (g.num_vars, g.claimed_sum, g.r_polys) == (w.num_vars, w.claimed_sum % R,
                                                              w.r_polys)
        for g, w in ((sp.opening_proof_denom_left, oproof.opening_proof_denom_left),
                     (sp.opening_proof_denom_right, oproof.opening_proof_denom_right)):
            assert (g.evaluation_point, g.evaluation, g.s_comm) == (w.evaluation_point,
                                                                    w.evaluation, w.s_comm)
            for k in ("poly_opening", "poly_opening_inv", "s_opening", "s_opening_inv"):
                assert (getattr(g, k).x, getattr(g, k).y, getattr(g, k).proof) == \
                    tuple(getattr(w, k))
        assert polys == [p[rank * L:(rank + 1) * L] for p in ods.polynomials]
        assert nvirt == len(ods.virtual_polys)
    proof, (pl, pr) = outs[0][0], outs[0][1]
    kzg = KZG.verifier(TAU)
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


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_lookup_prove_rejects_row_outside_table(world):
    """source row 41 is in no table row: QG_ERR_ASSERT naming it on every rank,
    before the prover touches the transcript or the stores"""
    from quill_amd import KZG, QuillGpuError, Transcript
    from quill_amd.logup import LookupProof
    lists = _xor_lists(bad_row=41)

    def fn(dev, rank, world):
        ss, ds, sc, dc = _sharded_stores(dev, rank, world, lists)
        kzg = KZG.trusted_setup(1 << 8, TAU, dev)
        t = Transcript(b"lookup")
        before = bytes(t.state)
        try:
            LookupProof.prove(ss, sc, ds, dc, None, t, kzg)
            res = None
        except QuillGpuError as e:
            res = (e.code, str(e))
        kzg.close()
        return res, bytes(t.state) == before, len(ds.polynomials), len(ds.virtual_polys)

    for res, untouched, npoly, nvirt in run_ranks(world, fn):
        assert res is not None and res[0] == -5 and "41" in res[1]
        assert untouched and (npoly, nvirt) == (2, 2)
