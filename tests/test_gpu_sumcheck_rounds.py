"""Sumcheck large rounds: every kernel and every expression shape, bit for bit.

run_rounds picks per call a template instance <K,NP>, a large-round kernel
(k_sc_big<K,4,true> for a product of distinct tables, k_sc_big<4,4,false> for
any other expression of <= 4 tables and degree <= 3, the LDS-staged
k_sc_round<K,NP> for the rest), a tail (k_sc_slice or k_sc_tail) and the round
the tail starts at, whose parity picks one of two limb accumulators.  By
default the large rounds need nvars >= 15..17; QG_SC_PERS_LOG (read per call)
lowers that, so nvars 9..13 give 3..7 large rounds over 1..16 blocks and the
Python oracle stays affordable.

Every case proves through the C-ABI on host tables and compares the round
messages with their trimmed lengths, the point, the final evaluation and the
transcript state with o.SumcheckProof.prove_fast on the same tables: equality,
no tolerance.  Before that it asserts from the context's path counters
(qg_ctx_counter) that the intended kernel ran the intended number of rounds
and that the tail started at the intended round, so a dispatch change cannot
move a case off its kernel unnoticed.

The default-threshold cases at the end (no switch set) use device tables and
the evaluation-form C oracle (oc_sumcheck_eval_expr, pinned on the CPU in
test_oracle_c.py)."""
import contextlib
import functools
import os

import pytest

import quill_oracle as o
import sumcheck_cases as sc

pytestmark = pytest.mark.gpu
R = o.R_MOD

SWITCHES = ("QG_SC_PERS_LOG", "QG_SC_BIG_BLOCKS", "QG_SC_BLOCKS", "QG_SC_STAGED",
            "QG_SC_NO_SKIP0", "QG_SC_OLD_TAIL")
COUNTERS = ("sc_big_pure_rounds", "sc_big_sop_rounds", "sc_staged_rounds", "sc_slice_tails",
            "sc_stream_tails", "sc_generic_calls")
KERNEL_COUNTER = {"pure": "sc_big_pure_rounds", "sop": "sc_big_sop_rounds",
                  "staged": "sc_staged_rounds"}
PERS = 6  # QG_SC_PERS_LOG of the small-shape cases: tables of > 2^6 entries are large rounds


@contextlib.contextmanager
def switches(**kw):
    """exactly the given QG_SC_* switches for the duration (PERS_LOG=6 -> QG_SC_PERS_LOG=6);
    every other one is unset, whatever the caller's environment holds"""
    want = {"QG_SC_" + k: str(v) for k, v in kw.items()}
    assert set(want) <= set(SWITCHES), want
    old = {n: os.environ.get(n) for n in SWITCHES}
    for n in SWITCHES:
        os.environ.pop(n, None)
    os.environ.update(want)
    try:
        yield
    finally:
        for n, v in old.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v


def snapshot(dev):
    return {n: dev.counter(n) for n in COUNTERS}


def assert_path(dev, before, kernel, rounds, tail="slice"):
    """counter differences of one call: `rounds` large rounds, all by `kernel`,
    the tail starting right after them, one tail launch of the given kind"""
    after = snapshot(dev)
    diff = {n: after[n] - before[n] for n in COUNTERS}
    want = dict.fromkeys(COUNTERS, 0)
    want[KERNEL_COUNTER[kernel]] = rounds
    want["sc_slice_tails" if tail == "slice" else "sc_stream_tails"] = 1
    assert diff == want
    assert dev.counter("sc_tail_first_round") == rounds


def prove(dev, nv, tabs, case, claimed, label=b"rounds", zerocheck=False):
    import quill_amd as q
    from quill_amd.hyperplonk import VirtualPolyExpr as E, sumcheck_prove_tables
    t = q.Transcript(label)
    rp, pt, ev = sumcheck_prove_tables(dev, nv, [list(tb) for tb in tabs],
                                       case.build(E.Input, E.Const), claimed, t, zerocheck)
    return rp, pt, ev, t.state


@functools.lru_cache(maxsize=None)
def reference(name, nv, kind="random", label=b"rounds"):
    """(tables, claimed sum, prove_fast's proof) of a case: computed once, shared
    by every test that proves the same input through another path"""
    case = sc.BY_NAME[name]
    tabs = sc.tables(nv, case.ntab) if kind == "random" else sc.degenerate_tables(kind, nv, case.ntab)
    claimed = sc.true_sum(case, tabs)
    if kind == "false_claim":
        claimed = (claimed + 1) % R
    return tabs, claimed, sc.oracle_prove(nv, tabs, sc.oracle_expr(case), claimed, label)


def check_case(dev, name, nv, kind="random", pers=PERS, tail="slice", kernel=None, **sw):
    case = sc.BY_NAME[name]
    tabs, claimed, want = reference(name, nv, kind)
    before = snapshot(dev)
    with switches(PERS_LOG=pers, **sw):
        got = prove(dev, nv, tabs, case, claimed)
    assert_path(dev, before, kernel or case.kernel, nv - pers, tail)
    assert [len(m) for m in got[0]] == [len(m) for m in want[0]]
    assert got == want
    return got


# --- per-kernel matrix ---------------------------------------------------------
# nvars 9 / 12 / 13 at QG_SC_PERS_LOG=6: 3 / 6 / 7 large rounds, the first over
# 1 / 8 / 16 blocks of 256 pairs, the last over 64 pairs (a quarter of a block)
MATRIX = [c.name for c in sc.CASES if not c.name.startswith("fac_")]


@pytest.mark.parametrize("nv", [9, 12, 13])
@pytest.mark.parametrize("name", MATRIX)
def test_large_rounds_match_oracle(dev, name, nv):
    check_case(dev, name, nv)


def test_matrix_covers_every_instance():
    """the matrix holds each <K,NP> instance of run_rounds and each k_sc_big form"""
    assert {(c.kernel, c.knp) for c in sc.CASES} >= {
        ("pure", (4, 4)), ("sop", (4, 4)), ("staged", (8, 4)), ("staged", (4, 8)),
        ("staged", (8, 8)), ("staged", (8, 16))}


# --- zero-check entry ----------------------------------------------------------
# h * eq has one more table and one more degree than h: g0 g1 eq is a product
# (pure), (3 g0 + g1) eq a 3-table expression of degree 2 (sop), the 5-table
# degree-3 expression becomes 6 tables at degree 4 (k_sc_round<8,8>)
@pytest.mark.parametrize("name,kernel", [("prod2", "pure"), ("deg1", "sop"), ("k5d3", "staged")])
def test_zerocheck_large_rounds_match_oracle(dev, name, kernel):
    nv = 12
    case = sc.BY_NAME[name]
    tabs = sc.tables(nv, case.ntab, seed=2)
    st = o.VirtualPolynomialStore(nv)
    for t in tabs:
        st.allocate_polynomial(list(t))
    h = st.new_virtual_from_expr(sc.oracle_expr(case))
    ot = o.Transcript(b"rounds-zc")
    oproof, (opt, oev) = o.ZeroCheckProof.prove(st, h, ot)
    before = snapshot(dev)
    with switches(PERS_LOG=PERS):
        got = prove(dev, nv, tabs, case, 0, b"rounds-zc", zerocheck=True)
    assert_path(dev, before, kernel, nv - PERS)
    assert got == (oproof.sumcheck_proof.r_polys, opt, oev, ot.state)


# --- grid edges ----------------------------------------------------------------
# nvars 12: 2048 pairs in round 0.  1 block: pure grid stride; 3 and 5: fewer
# than the 8 accumulator shards, and uneven shares; 8: one block per shard
@pytest.mark.parametrize("blocks", [1, 3, 5, 8])
@pytest.mark.parametrize("name", ["prod3", "mixed"])
def test_big_blocks_grid_edges(dev, name, blocks):
    check_case(dev, name, 12, BIG_BLOCKS=blocks)


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("name", ["k8d3", "k4d7"])
def test_staged_blocks_grid_edges(dev, name, blocks):
    check_case(dev, name, 12, BLOCKS=blocks)


# --- accumulator parity --------------------------------------------------------
# the tail reads the limb accumulator a0 (per-call header) when it starts at an
# even round and a1 (scratch that survives between calls) at an odd one
@pytest.mark.parametrize("old_tail", [False, True])
@pytest.mark.parametrize("pers", [6, 7])
@pytest.mark.parametrize("name", ["prod3", "mixed", "k4d7", "k8d3"])
def test_tail_start_parity(dev, name, pers, old_tail):
    nv = 12  # the tail starts at round 6 (even) or 5 (odd)
    if old_tail:
        check_case(dev, name, nv, pers=pers, tail="stream", OLD_TAIL=1)
    else:
        check_case(dev, name, nv, pers=pers)


# --- trimming and degenerate tables ---------------------------------------------
@pytest.mark.parametrize("kind", ["const_bit0", "const_bits01", "zero_factor", "small_values",
                                  "false_claim"])
@pytest.mark.parametrize("name", ["fac_sop", "fac_k4d4"])
def test_trimmed_messages_match_oracle(dev, name, kind):
    nv = 12
    got = check_case(dev, name, nv, kind=kind)
    lens = [len(m) for m in got[0]]
    full = sc.BY_NAME[name].degree + 1
    if kind == "zero_factor":
        assert lens == [0] * nv
    if kind == "const_bit0":
        assert lens[0] < full and lens[1:] == [full] * (nv - 1)
    if kind == "const_bits01":
        assert lens[0] < full and lens[1] < full and lens[2:] == [full] * (nv - 2)


# --- cross-checks between paths -------------------------------------------------
@pytest.mark.parametrize("name", ["prod3", "mixed"])
def test_staged_switch_matches_default(dev, name):
    """QG_SC_STAGED moves a k_sc_big expression to k_sc_round<4,4>: equal bytes"""
    a = check_case(dev, name, 12)
    b = check_case(dev, name, 12, kernel="staged", STAGED=1)
    assert a == b


@pytest.mark.parametrize("name", ["prod3", "mixed", "deg1", "const"])
def test_no_skip0_matches_default(dev, name):
    """h(0) from the claim (default, rounds >= 1) against h(0) evaluated"""
    a = check_case(dev, name, 12)
    b = check_case(dev, name, 12, NO_SKIP0=1)
    assert a == b


# --- call order in one context ---------------------------------------------------
def test_call_sequence_leaves_no_state(dev):
    """pure / sop / staged, odd / even tail start, nvars 13 / 9 / 12, 3 / 8
    tables, slice / streaming tail, back to back in one context: the oracle is
    stateless, so a stale a1, barrier shard or ticket shows as a mismatch"""
    seq = [("prod3", 13, 6, {}),        # pure, tail from round 7 (a1)
           ("k8d3", 9, 6, {}),          # staged, 8 tables, round 3 (a1, cleared by the host)
           ("mixed", 12, 6, {}),        # sop, round 6 (a0)
           ("k8d12", 12, 7, {}),        # staged <8,16>, round 5
           ("prod3", 12, 7, {"OLD_TAIL": 1}),   # pure, round 5, streaming tail
           ("mixed", 13, 6, {"BIG_BLOCKS": 3}),  # sop, round 7, 3 of 8 shards used
           ("k4d7", 12, 6, {"OLD_TAIL": 1}),    # staged, round 6, streaming tail
           ("prod3", 9, 6, {}),         # pure, one block, round 3
           ("mixed", 12, 7, {})]        # sop, round 5
    for name, nv, pers, sw in seq:
        check_case(dev, name, nv, pers=pers, tail="stream" if "OLD_TAIL" in sw else "slice", **sw)


# --- sharded large rounds ----------------------------------------------------------
# On a sharded context QG_SC_PERS_LOG also lowers the gather point: the ranks
# run js = min(nvars + 1 - PERS_LOG, nvars - log2(world)) large rounds on their
# local blocks (k_sc_finish after each), gather, and run the tail from round js.
def sharded_calls(world, pers, calls, **sw):
    """`calls` = [(case name, nvars)] proved in order by every rank of one
    loopback group, each rank in one context; per rank and call the proof, the
    counter differences and the tail's first round"""
    from test_gpu_multirank import run_ranks
    refs = [reference(name, nv) for name, nv in calls]

    def fn(dev, rank, world):
        out = []
        for (name, nv), (tabs, claimed, _) in zip(calls, refs):
            nl = (1 << nv) // world
            before = snapshot(dev)
            got = prove(dev, nv, [tb[rank * nl:(rank + 1) * nl] for tb in tabs], sc.BY_NAME[name],
                        claimed)
            after = snapshot(dev)
            out.append((got, {n: after[n] - before[n] for n in COUNTERS},
                        dev.counter("sc_tail_first_round")))
        return out
    with switches(PERS_LOG=pers, **sw):
        return run_ranks(world, fn), refs


def check_sharded(world, pers, calls, js, tail=None, **sw):
    outs, refs = sharded_calls(world, pers, calls, **sw)
    assert len(outs) == world
    for rank_out in outs:
        for (name, nv), (_, _, want), (got, diff, first), j in zip(calls, refs, rank_out, js):
            big = diff.pop(KERNEL_COUNTER[sc.BY_NAME[name].kernel])
            tails = (diff.pop("sc_slice_tails"), diff.pop("sc_stream_tails"))
            assert big == j and first == j
            assert sum(tails) == 1 and (tail is None or tails == ((1, 0) if tail == "slice" else (0, 1)))
            assert not any(diff.values())
            assert got == want


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("name", ["prod3", "mixed", "k8d3", "k4d7"])
def test_sharded_large_rounds_match_oracle(name, world):
    """nvars 12 at PERS_LOG 6: 7 large rounds on local blocks of 2^11 / 2^10
    entries (pure, sop, staged <8,4> and <4,8>), the tail from the odd round 7"""
    check_sharded(world, 6, [(name, 12)], [7])


def test_sharded_large_rounds_streaming_tail():
    check_sharded(2, 6, [("prod3", 12)], [7], tail="stream", OLD_TAIL=1)


@pytest.mark.parametrize("name", ["prod2", "mixed"])
def test_sharded_gather_round_clamp(name):
    """world 4, nvars 8, PERS_LOG 2: nvars + 1 - 2 = 7 exceeds the m = 6 local
    rounds, so js = 6 and the last sharded round has one local pair"""
    check_sharded(4, 2, [(name, 8)], [6])


def test_sharded_staged_then_pure_in_one_context():
    """staged large rounds, the tail from the odd round 7 (the scratch
    accumulator slot), then a product in the same contexts: what the staged
    rounds leave in the slot must not reach either tail"""
    check_sharded(2, 6, [("k8d3", 12), ("prod3", 12), ("k4d7", 12), ("mixed", 12)], [7, 7, 7, 7])


# --- switch values ---------------------------------------------------------------
@pytest.mark.parametrize("var,value", [
    ("PERS_LOG", "0"), ("PERS_LOG", "31"), ("PERS_LOG", "-3"), ("PERS_LOG", "six"),
    ("PERS_LOG", "6x"), ("PERS_LOG", ""), ("PERS_LOG", "6.5"),
    ("BIG_BLOCKS", "0"), ("BIG_BLOCKS", "2049"), ("BIG_BLOCKS", "many"),
    ("BLOCKS", "0"), ("BLOCKS", "2049"), ("BLOCKS", "99999999999999999999")])
def test_bad_switch_value_is_invalid(dev, var, value):
    from quill_amd._lib import QuillGpuError
    case = sc.BY_NAME["prod2"]
    tabs = sc.tables(7, case.ntab)
    before = snapshot(dev)
    with switches(**{var: value}):
        with pytest.raises(QuillGpuError) as e:
            prove(dev, 7, tabs, case, 1)
    assert e.value.code == -1  # QG_ERR_INVALID
    assert snapshot(dev) == before


def test_switch_range_ends_are_valid(dev):
    case = sc.BY_NAME["prod2"]
    tabs, claimed, want = reference("prod2", 9)
    for sw in ({"PERS_LOG": 30}, {"PERS_LOG": 6, "BIG_BLOCKS": 2048},
               {"PERS_LOG": 6, "STAGED": 1, "BLOCKS": 2048}):
        with switches(**sw):
            assert prove(dev, 9, tabs, case, claimed) == want
    tabs, claimed, want = reference("prod2", 1)  # 2 entries: no large round at 2^1 either
    with switches(PERS_LOG=1):
        assert prove(dev, 1, tabs, case, claimed) == want


# --- default thresholds (no switch set) ------------------------------------------
def _device_case(dev, name, nv, seed):
    """device tables from fill_random, proved with no switch set; the reference
    is the C evaluation-form oracle on the same Montgomery words"""
    import oracle_c as oc
    import quill_amd as q
    from quill_amd.hyperplonk import VirtualPolyExpr as E, _unpack_dev, sumcheck_prove_device
    case = sc.BY_NAME[name]
    tabs = [q.DeviceVec(dev, 1 << nv).fill_random(seed + i) for i in range(case.ntab)]
    host = [t.to_numpy() for t in tabs]
    expr = case.build(E.Input, E.Const)
    t = q.Transcript(b"rounds-dev")
    before = snapshot(dev)
    with switches():
        raw = sumcheck_prove_device(dev, nv, tabs, expr, 4242, t)
    after = snapshot(dev)
    for tb in tabs:
        tb.close()
    got = _unpack_dev(nv, expr, *raw) + (t.state,)
    want = oc.sumcheck_expr(nv, host, sc.oracle_expr(case), 4242,
                            o.Transcript(b"rounds-dev").state, mont=True)
    return case, {n: after[n] - before[n] for n in COUNTERS}, got, want


@pytest.mark.parametrize("name,nv", [("mixed", 18), ("k8d3", 16), ("k4d7", 17), ("k8d12", 16)])
def test_default_thresholds_match_c_oracle(dev, name, nv):
    """The split between large rounds and tail is the device's (PERS_LOG = 16,
    lowered to what the slice tail holds for this <K,NP>): the counters' own
    rule is asserted, i.e. every round before the tail's first ran the case's
    kernel, there is at least one, and nothing else ran."""
    case, diff, got, want = _device_case(dev, name, nv, 900 + nv)
    j0 = dev.counter("sc_tail_first_round")
    assert 1 <= j0 <= nv - 1
    assert nv - j0 <= 16  # the tail never starts above 2^PERS_LOG entries
    big = diff.pop(KERNEL_COUNTER[case.kernel])
    tails = diff.pop("sc_slice_tails") + diff.pop("sc_stream_tails")
    assert (big, tails) == (j0, 1)
    assert not any(diff.values())
    assert [len(m) for m in got[0]] == [len(m) for m in want[0]]
    assert got == want


def test_unset_environment_path_at_2p20(dev):
    """No switch set, h = g0 g1 g2 at 2^20: k_sc_big<4,4,true> runs rounds 0..3
    and the slice tail takes over at 2^16 entries, as before the switches were
    read per call."""
    import quill_amd as q
    from quill_amd.hyperplonk import VirtualPolyExpr as E, sumcheck_prove_device
    nv = 20
    tabs = [q.DeviceVec(dev, 1 << nv).fill_random(77 + i) for i in range(3)]
    before = snapshot(dev)
    with switches():
        sumcheck_prove_device(dev, nv, tabs, E.Input(0) * E.Input(1) * E.Input(2), 1,
                              q.Transcript(b"p20"))
    for tb in tabs:
        tb.close()
    assert_path(dev, before, "pure", 4)
