"""Lookup multiplicities with a hash-partitioned table on sharded contexts
(qg_lookup_multiplicities_dev_ex with QG_LOOKUP_TABLE_PARTITIONED,
csrc/lookup.hip lookup_run_partitioned) and LookupProof.prove(...,
table="partitioned") on sharded device stores.

Ranks run as threads on one GPU over the in-process loopback communicator.
Rank r holds rows [r L, (r + 1) L) of every column; the expected column is a
dict count over the concatenated blocks, written here: m[j] = number of global
source rows equal to global table row j, a tuple the table holds at several
rows counted at the lowest of them.  Every parity case also compares the block
with the replicated mode's block from the same contexts.  Columns are raw
(n, 4) uint64 Montgomery arrays."""
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
REPLICATED, PARTITIONED = 0, 1
LDS_ROWS = 16384  # csrc/lookup.hip LK_LDS_ROWS: per-block LDS counters up to here
COUNTERS = ("lookup_collectives", "lookup_routed_tab", "lookup_routed_src",
            "lookup_exchange_bytes")


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


def _call(dev, src, tab, mode=PARTITIONED, ns=None, nt=None):
    """src / tab: DeviceVec lists -> (rc, block words or None, first_missing)"""
    from quill_amd import DeviceVec, lib
    ns = src[0].n if ns is None else ns
    nt = tab[0].n if nt is None else nt
    o_ = DeviceVec(dev, max(tab[0].n, 1))
    miss = C.c_int64(-7)
    sp = (C.c_void_p * len(src))(*[v.h.value for v in src])
    tp = (C.c_void_p * len(tab))(*[v.h.value for v in tab])
    rc = lib().qg_lookup_multiplicities_dev_ex(dev.h, len(src), sp, ns, tp, nt, o_.h,
                                               C.byref(miss), mode)
    res = o_.to_numpy(nt) if rc == 0 else None
    o_.close()
    return rc, res, miss.value


def _counters(dev):
    return {k: dev.counter(k) for k in COUNTERS}


def _delta(dev, before):
    return {k: dev.counter(k) - before[k] for k in COUNTERS}


def _last_error(dev):
    from quill_amd import lib
    return lib().qg_last_error(dev.h).decode()


def _run(world, src, tab, modes=(PARTITIONED, REPLICATED)):
    """one call per mode on the same contexts -> per rank a list of
    (rc, block, first_missing, counter deltas), in the order of `modes`"""
    def fn(dev, rank, world):
        ds = [_upload(dev, a) for a in _block(src, rank, world)]
        dt = [_upload(dev, a) for a in _block(tab, rank, world)]
        res = []
        for mode in modes:
            before = _counters(dev)
            rc, got, fm = _call(dev, ds, dt, mode)
            res.append((rc, got, fm, _delta(dev, before)))
        for v in ds + dt:
            v.close()
        return res
    return run_ranks(world, fn)


def _check(world, src, tab):
    """every rank's partitioned block against the slice of the dict count and
    against the replicated block; 6 collectives; returns (m, per-rank deltas of
    the partitioned call)"""
    m, miss = _expected(src, tab)
    assert miss == -1 and sum(m) == src[0].shape[0]
    want = _mont(m)
    L = len(m) // world
    deltas = []
    for rank, (part, repl) in enumerate(_run(world, src, tab)):
        assert (part[0], part[2]) == (0, -1), rank
        assert (repl[0], repl[2]) == (0, -1), rank
        assert np.array_equal(part[1], want[rank * L:(rank + 1) * L]), rank
        assert np.array_equal(part[1], repl[1]), rank
        assert part[3]["lookup_collectives"] == 6
        assert repl[3]["lookup_collectives"] == len(src) + 3
        deltas.append(part[3])
    return m, deltas


def _table(nt, ncols):
    """nt distinct rows of ncols columns"""
    j = np.arange(nt)
    if ncols == 1:
        return [_mont(j)]
    return [_mont(j % 7), _mont(j // 7), _mont((j * j) % 5)][:ncols]


def _pick(tab, idx):
    return [np.ascontiguousarray(t[idx]) for t in tab]


# ---- parity and ownership ----------------------------------------------------
@pytest.mark.parametrize("ncols", [1, 3])
@pytest.mark.parametrize("world", [2, 4, 8])
def test_blocks_equal_global_count(world, ncols):
    """global table of 64 rows, 100 source rows per rank; exactly 6 collectives"""
    tab = _table(64, ncols)
    rnd = random.Random(world * 10 + ncols)
    idx = [rnd.randrange(64) for _ in range(100 * world)]
    m, deltas = _check(world, _pick(tab, idx), tab)
    assert max(m) > 1
    # every distinct row of a block travels once
    for rank, d in enumerate(deltas):
        assert d["lookup_routed_tab"] == 64 // world
        assert d["lookup_routed_src"] == len(set(idx[rank * 100:(rank + 1) * 100]))


def test_lengths_off_every_block_size():
    """257 table rows and 1025 source rows per rank: no multiple of a block, a
    wave or the even chunk length"""
    world = 2
    tab = _table(257 * world, 3)
    rnd = random.Random(257)
    _check(world, _pick(tab, [rnd.randrange(257 * world) for _ in range(1025 * world)]), tab)


def test_one_table_row_per_rank():
    tab = _table(8, 3)
    rnd = random.Random(8)
    _check(8, _pick(tab, [rnd.randrange(8) for _ in range(8 * 33)]), tab)


def test_duplicate_rows_across_ranks():
    """a tuple at global rows 3 (rank 0) and 10 (rank 1) is counted at row 3;
    one at rows 12 and 14 (both rank 1) at row 12"""
    a = list(range(16))
    a[10] = a[3]
    a[14] = a[12]
    tab = [_mont(a), _mont([x * x % 97 for x in a])]
    idx = [3, 10, 10, 12, 14, 14, 14, 0, 15, 10] + [10, 3, 14, 12, 7, 7, 3, 10, 14, 1]
    m, _ = _check(2, _pick(tab, idx), tab)
    assert m[10] == m[14] == 0
    assert m[3] == idx.count(3) + idx.count(10) and m[12] == idx.count(12) + idx.count(14)


def test_counts_travel_to_the_holding_rank():
    """rank r's source rows all lie in rank (r + 1) mod W's table block: the
    counts must reach the rank that holds the row, not stay with the owner"""
    world, L, S = 4, 16, 50
    tab = _table(world * L, 3)
    rnd = random.Random(77)
    idx = []
    for r in range(world):
        nxt = (r + 1) % world
        idx += [nxt * L + rnd.randrange(L) for _ in range(S)]
    m, _ = _check(world, _pick(tab, idx), tab)
    assert all(sum(m[r * L:(r + 1) * L]) == S for r in range(world))


# ---- dedup and skew ------------------------------------------------------------
def test_one_source_tuple_is_one_record_per_rank():
    world = 4
    tab = _table(64, 2)
    m, deltas = _check(world, _pick(tab, [37] * (world * 300)), tab)
    assert m[37] == world * 300
    assert [d["lookup_routed_src"] for d in deltas] == [1] * world
    assert [d["lookup_routed_tab"] for d in deltas] == [16] * world


def test_one_table_tuple_is_one_record_per_rank():
    """the table is one row repeated: one record per rank, the lowest global row
    takes everything"""
    world = 4
    tab = [_mont([5] * 64), _mont([9] * 64)]
    m, deltas = _check(world, _pick(tab, [0] * (world * 77)), tab)
    assert m[0] == world * 77 and not any(m[1:])
    assert [d["lookup_routed_tab"] for d in deltas] == [1] * world
    assert [d["lookup_routed_src"] for d in deltas] == [1] * world


@pytest.mark.parametrize("env", [{"QG_LOOKUP_OWNER_BITS": "0"}, {"QG_LOOKUP_HASH_BITS": "0"},
                                 {"QG_LOOKUP_OWNER_BITS": "0", "QG_LOOKUP_HASH_BITS": "0"}])
def test_skew_switches_change_no_result(monkeypatch, env):
    """every record on rank 0, every record in one probe chain, and both"""
    tab = _table(64, 3)
    rnd = random.Random(5)
    src = _pick(tab, [rnd.randrange(64) for _ in range(400)])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check(4, src, tab)


# ---- size and determinism ----------------------------------------------------
@pytest.fixture(scope="module")
def big_case():
    """2^15 global table rows at world 4 (above LK_LDS_ROWS), 2^12 source rows
    per rank, half of them on one table row"""
    world, nt = 4, 1 << 15
    tab = _table(nt, 2)
    rnd = np.random.RandomState(nt)
    ns = world << 12
    idx = rnd.randint(0, nt, size=ns)
    idx[rnd.rand(ns) < 0.5] = nt // 3
    idx[:4] = [0, nt - 1, nt - 1, LDS_ROWS - 1]  # the edge rows are hit
    return world, _pick(tab, idx), tab


def test_table_above_the_lds_limit(big_case):
    world, src, tab = big_case
    m, _ = _check(world, src, tab)
    assert max(m) > (world << 12) // 3


def test_same_call_twice_gives_identical_blocks(big_case):
    world, src, tab = big_case
    outs = _run(world, src, tab, modes=(PARTITIONED, PARTITIONED))
    for a, b in outs:
        assert (a[0], b[0]) == (0, 0) and np.array_equal(a[1], b[1])
        assert a[3] == b[3]


# ---- errors and agreement ----------------------------------------------------
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


@pytest.mark.parametrize("how", ["mode", "tab_len", "unknown_mode"])
def test_ranks_that_disagree_all_return_invalid(how):
    """rank 1 passes the other mode, another tab_len, or a mode that does not
    exist: every rank returns QG_ERR_INVALID and none waits in a collective; the
    next call on the same contexts is right"""
    world, L = 4, 16
    tab = _table(world * L, 2)
    rnd = random.Random(31)
    src = _pick(tab, [rnd.randrange(world * L) for _ in range(world * 20)])
    want = _mont(_expected(src, tab)[0])

    def fn(dev, rank, world):
        ds = [_upload(dev, a) for a in _block(src, rank, world)]
        dt = [_upload(dev, a) for a in _block(tab, rank, world)]
        odd = rank == 1
        if how == "mode":
            rc = _call(dev, ds, dt, REPLICATED if odd else PARTITIONED)[0]
        elif how == "tab_len":
            rc = _call(dev, ds, dt, nt=L - 1 if odd else L)[0]
        else:
            rc = _call(dev, ds, dt, 7 if odd else PARTITIONED)[0]
        rc2, got, fm = _call(dev, ds, dt)
        for v in ds + dt:
            v.close()
        return rc, rc2, got, fm

    for rank, (rc, rc2, got, fm) in enumerate(run_ranks(world, fn)):
        assert rc == -1
        assert (rc2, fm) == (0, -1)
        assert np.array_equal(got, want[rank * L:(rank + 1) * L])


def test_unknown_mode_is_invalid(dev):
    """on a plain context and on every rank of a group"""
    col = _mont(range(8))
    ds, dt = [_upload(dev, col)], [_upload(dev, col)]
    assert _call(dev, ds, dt, 2)[0] == -1
    assert "mode" in _last_error(dev)
    assert _call(dev, ds, dt, 0xffffffff)[0] == -1
    for v in ds + dt:
        v.close()

    def fn(d, rank, world):
        s, t = [_upload(d, col)], [_upload(d, col)]
        rc = _call(d, s, t, 2)[0]
        rc2 = _call(d, s, t)[0]
        for v in s + t:
            v.close()
        return rc, rc2

    assert run_ranks(2, fn) == [(-1, 0)] * 2


# ---- collectives, caps and context kinds ----------------------------------------
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
        msg = _last_error(dev)
        c = _call(dev, ds, dt)[0]
        for v in ds + dt:
            v.close()
        return a, b, used, c, msg

    for a, b, used, c, msg in run_ranks(2, fn):
        assert (a, b, used, c) == (-4, -4, 2, 0)
        assert msg == "lookup multiplicities: 2^32 global source rows or more"


def _plain_and(dev, other, src, tab):
    """the partitioned call on a plain context and on `other`, with the plain
    replicated call -> [(rc, block, first_missing, deltas)] x 3"""
    res = []
    for d, mode in ((dev, REPLICATED), (dev, PARTITIONED), (other, PARTITIONED)):
        ds, dt = [_upload(d, a) for a in src], [_upload(d, a) for a in tab]
        before = _counters(d)
        rc, got, fm = _call(d, ds, dt, mode)
        res.append((rc, got, fm, _delta(d, before)))
        for v in ds + dt:
            v.close()
    return res


def test_plain_and_forced_one_rank_rccl_contexts(dev):
    """a context with no communicator runs the one-context flow in either mode
    (0 collectives); QG_FORCE_RCCL=1: a world-1 context with a real one-rank RCCL
    communicator goes through the partitioned flow (ncclAllGather, grouped
    send/recv) and equals it"""
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
    plain, plain_part, forced = _plain_and(dev, rdev, src, tab)
    rdev.close()
    for r in (plain, plain_part, forced):
        assert (r[0], r[2]) == (0, -1)
        assert np.array_equal(r[1], plain[1])
    assert np.array_equal(plain[1], _mont(_expected(src, tab)[0]))
    zero = {k: 0 for k in COUNTERS}
    assert plain[3] == zero and plain_part[3] == zero
    assert forced[3]["lookup_collectives"] == 6
    assert forced[3]["lookup_routed_tab"] == 300
    assert forced[3]["lookup_routed_src"] == len(set(_keys(src)))


# ---- traffic -------------------------------------------------------------------
@pytest.mark.parametrize("world", [4, 8])
def test_partitioned_receives_less_than_replicated(world):
    """table and source both 4096 distinct rows per rank, 2 columns.  Derived,
    not measured: a replicated call receives W x tab_len x (32 x ncols + 4)
    bytes per rank; a partitioned one W x (max_t x 76 + max_s x 72) with max the
    most records any rank sends any rank, at least L / W - so at least
    2 x 72 L + 4 L, and with an even hash little more (272 L replicated at
    W = 4)."""
    L, ncols = 4096, 2
    n = L * world
    j = np.arange(n)
    tab = [_mont(j % 181), _mont(j // 181)]
    perm = np.random.RandomState(world).permutation(n)
    src = _pick(tab, perm)
    outs = _run(world, src, tab)
    want = _mont([1] * n)
    replicated = world * L * (32 * ncols + 4)
    for rank, (part, repl) in enumerate(outs):
        assert (part[0], repl[0]) == (0, 0)
        assert np.array_equal(part[1], want[rank * L:(rank + 1) * L])
        assert np.array_equal(part[1], repl[1])
        assert part[3]["lookup_routed_tab"] == L and part[3]["lookup_routed_src"] == L
        got = part[3]["lookup_exchange_bytes"]
        print("world %d rank %d: partitioned %d B, replicated %d B, floor %d B"
              % (world, rank, got, repl[3]["lookup_exchange_bytes"], 2 * L * 72 + 4 * L))
        assert repl[3]["lookup_exchange_bytes"] == replicated
        assert 2 * L * 72 + 4 * L <= got < replicated
    # all ranks agreed on the chunk lengths
    assert len({p[3]["lookup_exchange_bytes"] for p, _ in outs}) == 1


# ---- LookupProof.prove(..., multiplicities=None, table="partitioned") ------------
def _xor_lists():
    """the XOR-42 shape: source 2^6 rows, table 2^8 rows"""
    rnd = random.Random(42)
    c1, c2 = list(range(256)), [i ^ 42 for i in range(256)]
    by = [rnd.randrange(256) for _ in range(1 << 6)]
    s1, s2 = list(by), [b ^ 42 for b in by]
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
    return oproof, pts, bytes(ot.state), ods


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
def test_sharded_lookup_prove_with_partitioned_table(world, xor_oracle):
    """every rank's proof, points and transcript state equal o.lookup_prove given
    the hand-counted column; LookupProof.verify accepts; the count used the
    partitioned flow (6 collectives, records routed)"""
    from quill_amd import KZG, EvaluationClaim, Transcript
    from quill_amd.logup import LookupProof
    oproof, (opl, opr), ostate, ods = xor_oracle
    lists = _xor_lists()
    s1, s2, c1, c2, mult = lists

    def fn(dev, rank, world):
        ss, ds, sc, dc = _sharded_stores(dev, rank, world, lists)
        kzg = KZG.trusted_setup(1 << 8, TAU, dev)
        t = Transcript(b"lookup")
        before = _counters(dev)
        proof, pts = LookupProof.prove(ss, sc, ds, dc, None, t, kzg, table="partitioned")
        used = _delta(dev, before)
        polys = [p.to_list() for p in ds.polynomials]
        kzg.close()
        return proof, pts, bytes(t.state), polys, used

    outs = run_ranks(world, fn)
    L = 256 // world
    for rank, (proof, (pl, pr), state, polys, used) in enumerate(outs):
        assert (pl, pr) == (opl, opr) and state == ostate
        assert used["lookup_collectives"] == 6 and used["lookup_routed_tab"] == L
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
    proof, (pl, pr) = outs[0][0], outs[0][1]
    kzg = KZG.verifier(TAU)
    vt = Transcript(b"lookup")
    proof.verify(vt, kzg,
                 [EvaluationClaim(pl, o.mle_evaluate(s1, pl)),
                  EvaluationClaim(pl, o.mle_evaluate(s2, pl))],
                 [EvaluationClaim(pr, o.mle_evaluate(c1, pr)),
                  EvaluationClaim(pr, o.mle_evaluate(c2, pr))],
                 EvaluationClaim(pr, o.mle_evaluate(mult, pr)))


def test_python_rejects_an_unknown_table_name(dev):
    from quill_amd import VirtualPolynomialStore, lookup_multiplicities
    st = VirtualPolynomialStore(2, dev)
    st.allocate_polynomial([1, 2, 3, 4])
    v = [st.new_virtual_from_input(0)]
    with pytest.raises(ValueError):
        lookup_multiplicities(st, v, st, v, dev, table="hashed")
    m = lookup_multiplicities(st, v, st, v, dev, table="partitioned")
    assert m.to_list() == [1, 1, 1, 1]
    m.close()
