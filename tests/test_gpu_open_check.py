"""The prover-side quotient check of every KZG opening (kzg.rs:85):
p(sigma) - y == q(sigma) (sigma - x) on the device at a random sigma that never
touches the transcript, p over the caller's untrimmed length.

  * the evaluation kernel (qg_poly_eval_dev) against the oracle's Horner;
  * the check runs, is silent on good proofs and changes no proof byte;
  * the test-only faults (qg_debug_open_fault) - a short trimmed length, a
    corrupted quotient coefficient, a poisoned trimmed-length stamp word - end
    in QG_ERR_ASSERT "Polynomial division failed" (the stamp: in a correct
    proof), and the context is clean afterwards;
  * zero tails across the trimmed-length scan's 16K tail boundary against the
    oracle verifier;
  * sharded contexts: every rank takes the same decision.
The switches are read per call, so the tests toggle them in-process."""
import contextlib
import os
import random
import threading

import numpy as np
import pytest

import quill_oracle as o

pytestmark = pytest.mark.gpu
R = o.R_MOD
TAU = 0x4F50454E434845434B
KEYS = ("poly_opening", "poly_opening_inv", "s_opening", "s_opening_inv")


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name)
        else:
            os.environ[name] = old


def counters(dev):
    return dev.counter("open_checks"), dev.counter("open_check_failures")


# ---------------------------------------------------------------- 1. the kernel
# thread strip 32, block span 8192 (256 strips), two blocks at 16384; 1024 is
# the 32 strips of half a wave; 40000 leaves a partial span and a partial strip
LENGTHS = [0, 1, 2, 31, 32, 33, 1023, 1024, 1025, 8191, 8192, 8193, 16383, 16384, 16385, 40000]


@pytest.fixture(scope="module")
def evec(dev):
    from quill_amd import DeviceVec
    v = DeviceVec(dev, 40000).fill_random(0xE7A1)
    arr = v.to_numpy()
    yield v, arr
    v.close()


def horner(arr, n, x, shift=0):
    import oracle_c as oc
    return (oc.fr_horner(arr[:n], x) if n else 0) * pow(x, shift, R) % R


@pytest.mark.parametrize("x", [0, 1, R - 1, 0x1D0C5EED0DDBA11 * 0x9E3779B97F4A7C15 % R])
def test_evaluate_matches_oracle_horner(evec, x):
    v, arr = evec
    for n in LENGTHS:
        assert v.evaluate(x, n) == horner(arr, n, x), n
    with env("QG_EVAL_BLOCKS", "2"):  # 5 spans on 2 blocks: the grid-stride loop wraps
        assert v.evaluate(x, 40000) == horner(arr, 40000, x)


@pytest.mark.parametrize("shift", [0, 1, 12345])
def test_evaluate_shift(evec, shift):
    v, arr = evec
    x = random.Random(shift).randrange(R)
    for n in (0, 33, 8193, 40000):
        assert v.evaluate(x, n, shift) == horner(arr, n, x, shift), n


def test_evaluate_zero_tail_and_views(dev):
    from quill_amd import DeviceVec
    v = DeviceVec(dev, 40000).fill_random(0xE7A2)
    DeviceVec.from_u64(dev, np.zeros(20000, dtype=np.uint64), out=v, offset=20000)
    arr = v.to_numpy()
    x = random.Random(5).randrange(R)
    assert v.evaluate(x) == horner(arr, 40000, x) == horner(arr, 20000, x)
    w = v.view(100, 10000)
    assert w.evaluate(x) == horner(arr[100:], 10000, x)
    v.close()


def test_evaluate_span_stage_strip_of_two(dev):
    """More than 256 first-stage spans (n > 2^21) is the smallest shape whose span
    stage leaves strip length 1: 2^21 + 8193 coefficients are 258 spans, strip 2.
    In the two-point call a 33-coefficient job (one span) shares that launch's
    strip length."""
    import oracle_c as oc
    from quill_amd import DeviceVec
    n = (1 << 21) + 8193
    v = DeviceVec(dev, n).fill_random(0xE7A3)
    w = DeviceVec(dev, 33).fill_random(0xE7A4)
    arr = v.to_numpy()
    xs = (random.Random(0xE7A5).randrange(2, R), R - 1)
    one = [v.evaluate(x, n) for x in xs]
    assert one == [oc.fr_horner(arr, x) for x in xs]
    assert dev.poly_eval2([v, w], [n, 33], xs) == [[y, w.evaluate(x)] for x, y in zip(xs, one)]
    with env("QG_EVAL_BLOCKS", "2"):  # 129 spans per block
        assert [v.evaluate(x, n) for x in xs] == one
    v.close()
    w.close()


def test_evaluate_rejects_a_length_past_the_buffer(dev):
    from quill_amd import DeviceVec
    from quill_amd._lib import QuillGpuError
    v = DeviceVec(dev, 8)
    with pytest.raises(QuillGpuError) as e:
        v.evaluate(3, 9)
    assert e.value.code == -1
    v.close()


# ---------------------------------------------------------------- shared openings
@pytest.fixture(scope="module")
def kzg(dev):
    from quill_amd import KZG
    k = KZG.trusted_setup(1 << 15, TAU, dev)
    yield k
    k.close()


@pytest.fixture(scope="module")
def vecs(dev):
    """full vectors (every coefficient nonzero: a dropped one changes p) and two zeros"""
    from quill_amd import DeviceVec
    d = {"full15": DeviceVec(dev, 1 << 15).fill_random(0xF15),
         "odd14": DeviceVec(dev, (1 << 14) + 3).fill_random(0xF14),
         "full12": DeviceVec(dev, 1 << 12).fill_random(0xF12),
         "full13": DeviceVec(dev, 1 << 13).fill_random(0xF13),
         "zero12": DeviceVec.from_u64(dev, np.zeros(1 << 12, dtype=np.uint64)),
         "tail12": DeviceVec(dev, 1 << 12).fill_random(0xF11),
         "one12": DeviceVec(dev, 1 << 12).fill_random(0xF10)}
    DeviceVec.from_u64(dev, np.zeros(1096, dtype=np.uint64), out=d["tail12"], offset=3000)
    DeviceVec.from_u64(dev, np.zeros(4095, dtype=np.uint64), out=d["one12"], offset=1)
    yield d
    for v in d.values():
        v.close()


def point(nv, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(nv)]


def batch_items(vecs, names, seed):
    out = []
    for i, nm in enumerate(names):
        n = len(vecs[nm])
        out.append((vecs[nm], n, point(max(1, (n - 1).bit_length()), seed + i), False))
    return out


UNI = [random.Random(77).randrange(1, R) for _ in range(20000)]


def do_uni(kzg, vecs):
    return kzg.open_univariate(UNI, 0xABCDEF0123456789), None


def do_dev(kzg, vecs, name="full15"):
    from quill_amd import Transcript
    t = Transcript(b"open-check")
    v = vecs[name]
    return kzg.open_dev(v, len(v), point((len(v) - 1).bit_length(), 11), t), t.state


def do_batch(kzg, vecs):
    """the first nonzero trimmed length (and the first non-empty quotient) is the
    third item's: the two before it are zero vectors"""
    from quill_amd import Transcript
    t = Transcript(b"open-check-batch")
    items = batch_items(vecs, ["zero12", "zero12", "full15", "full12", "full13"], 500)
    return kzg.open_batch_dev(items, t), t.state


PATHS = {"univariate": do_uni, "open_dev": do_dev, "batch": do_batch}


# ---------------------------------------------------------------- 2. silent on good proofs
def test_check_counts_and_leaves_proofs_unchanged(dev, kzg, vecs):
    from quill_amd import Transcript
    c0, f0 = counters(dev)
    uni = do_uni(kzg, vecs)
    assert counters(dev) == (c0 + 1, f0)
    one = do_dev(kzg, vecs)
    assert counters(dev) == (c0 + 5, f0)
    # trimmed lengths (poly, S) of the five items: 4096 / 4095, 3000 / 4095,
    # 1 / 4095 (S_k = g_{k+1} f_0), 0 / 0 and 8192 / 8191.  open_checks counts
    # every quotient whose polynomial has a nonzero trimmed length - also
    # one12's two poly quotients, which have no coefficient left (the check is
    # then p(sigma) == y) - so 4 per item but the zero vector, whose four
    # quotients do not exist (p(sigma) == 0 is checked there, not counted)
    names = ["full12", "tail12", "one12", "zero12", "full13"]

    def batch():
        t = Transcript(b"open-check-count")
        return kzg.open_batch_dev(batch_items(vecs, names, 900), t), t.state
    bat = batch()
    assert counters(dev) == (c0 + 5 + 16, f0)
    with env("QG_OPEN_CHECK", "0"):
        assert (do_uni(kzg, vecs), do_dev(kzg, vecs), batch()) == (uni, one, bat)
    assert counters(dev) == (c0 + 21, f0)  # switched off: nothing counted
    for seed in ("1", "0xfeedfacecafebeef"):
        with env("QG_OPEN_CHECK_SEED", seed):
            assert (do_uni(kzg, vecs), do_dev(kzg, vecs), batch()) == (uni, one, bat)
    assert counters(dev) == (c0 + 21 + 2 * 21, f0)


def test_zero_polynomial_is_checked_but_not_counted(dev, kzg):
    """trimmed length 0: no quotient to count; p(sigma) == 0 over all n entries
    is still checked and holds"""
    c0, f0 = counters(dev)
    op = kzg.open_univariate([0] * 5000, 12345)
    assert (op.y, op.proof) == (0, None)
    assert counters(dev) == (c0, f0)


# ---------------------------------------------------------------- 3 / 4. the faults are caught
def assert_caught(dev, kzg, vecs, run, kind, value, where):
    from quill_amd._lib import QuillGpuError
    want = run(kzg, vecs)
    c0, f0 = counters(dev)
    dev.debug_open_fault(kind, value)
    with pytest.raises(QuillGpuError) as e:
        run(kzg, vecs)
    assert e.value.code == -5
    assert "Polynomial division failed" in str(e.value)
    assert where in str(e.value), str(e.value)
    f1 = dev.counter("open_check_failures")
    assert f1 > f0
    assert run(kzg, vecs) == want  # the fault was one-shot: the context is clean
    assert dev.counter("open_check_failures") == f1


WHERE = {"univariate": "opening 0 of 1, quotient 0", "open_dev": "opening 0 of 1, quotient 0",
         "batch": "opening 2 of 5, quotient 0"}


@pytest.mark.parametrize("value", [1, 768, 16384])
@pytest.mark.parametrize("path", ["univariate", "open_dev", "batch"])
def test_short_trim_is_caught(dev, kzg, vecs, path, value):
    """the dropped coefficients are nonzero, so p(sigma) - y == q(sigma)(sigma - x)
    fails except with probability <= n / r; 768 is the round-5 shortfall"""
    assert_caught(dev, kzg, vecs, PATHS[path], 1, value, WHERE[path])


@pytest.mark.parametrize("index", [0, (1 << 14) + 1, 7777])
def test_corrupt_quotient_is_caught_open_dev(dev, kzg, vecs, index):
    """n = 2^14 + 3: the quotient has 2^14 + 2 coefficients (first, last, middle)"""
    assert_caught(dev, kzg, vecs, lambda k, v: do_dev(k, v, "odd14"), 2, index,
                  "opening 0 of 1, quotient 0")


def test_corrupt_quotient_is_caught_batch(dev, kzg, vecs):
    assert_caught(dev, kzg, vecs, do_batch, 2, 12345, WHERE["batch"])


def test_disarm(dev, kzg, vecs):
    want = do_dev(kzg, vecs)
    dev.debug_open_fault(1, 5)
    dev.debug_open_fault(0)
    assert do_dev(kzg, vecs) == want


# ---------------------------------------------------------------- 5 / 6. zero tails, the stamp word
def open_zero_tailed(dev, n, live, before=None):
    """open_dev of n entries, the first `live` random, checked by the oracle
    verifier (mlpcs.rs:126-161, KZG by the trapdoor identity)"""
    import oracle_c as oc
    from quill_amd import KZG, DeviceVec, Transcript
    nv = (n - 1).bit_length()
    kz = KZG.trusted_setup(1 << nv, TAU, dev)
    v = DeviceVec(dev, n).fill_random(0x7A11 + live)
    DeviceVec.from_u64(dev, np.zeros(n - live, dtype=np.uint64), out=v, offset=live)
    arr = v.to_numpy()
    pt = point(nv, n + live)
    if before:
        before()
    t = Transcript(b"zero-tail")
    proof = kz.open_dev(v, n, pt, t)
    v.close()
    kz.close()
    C = oc.g1_mul(o.G1_GEN, oc.fr_horner(arr, TAU))
    ext = np.vstack([arr, np.zeros(((1 << nv) - n, 4), dtype=np.uint64)]) if (1 << nv) > n else arr
    assert proof.evaluation == oc.fr_mle_eval(ext, pt)
    op = o.MLEvalProof(pt, proof.evaluation, proof.s_comm,
                       *[(getattr(proof, k).x, getattr(proof, k).y, getattr(proof, k).proof)
                         for k in KEYS])
    vt = o.Transcript(b"zero-tail")
    assert op.verify(C, o.KZG(1 << nv, TAU, points=[]), vt)
    assert vt.state == t.state
    return proof


@pytest.mark.parametrize("n,live", [(40000, 20000), (40000, 23616), (40000, 23617),
                                    (32768, 16384), (32768, 16385), (32768, 1), (16385, 1)])
def test_zero_tail_across_the_16k_boundary(dev, n, live):
    """the trimmed-length scan's body launch with an all-zero / a barely
    nonzero 16K tail (n - 16384 = 23616 at n = 40000)"""
    f0 = dev.counter("open_check_failures")
    open_zero_tailed(dev, n, live)
    assert dev.counter("open_check_failures") == f0


@pytest.mark.parametrize("g", [1, 0xFFFFFF])
def test_poisoned_stamp_word(dev, g):
    """a stamp word that claims a nonzero tail (in the old encoding: for
    generation g) must not make the body scan skip: the length would come out
    short, which the quotient check reports; with the word zeroed before every
    tail launch the proof is the unpoisoned one"""
    want = open_zero_tailed(dev, 40000, 20000)
    got = open_zero_tailed(dev, 40000, 20000,
                           before=lambda: dev.debug_open_fault(3, (g << 40) | 12345))
    assert got == want


# ---------------------------------------------------------------- 7. sharded
NV = 9


def sharded_case(world, arm=None, seed=40):
    """test_sharded_mle_open's shape; arm(rank) -> (kind, value) or None.
    Returns the reference proof / state and per rank (proof, state, checks) or
    the error code."""
    import quill_amd as q
    from quill_amd import KZG, Transcript
    from quill_amd._lib import QuillGpuError
    from test_gpu_multirank import run_ranks
    rnd = random.Random(seed + world)
    N = 1 << NV
    L = N // world
    tau = rnd.randrange(R)
    poly = [rnd.randrange(1, R) for _ in range(N)]
    pt = [rnd.randrange(R) for _ in range(NV)]
    dev0 = q.Device(0)
    ref_kzg = KZG.trusted_setup(N, tau, dev0)
    t_ref = Transcript(b"shard-check")
    ref = ref_kzg.open(poly, pt, t_ref)
    ref_kzg.srs.close()
    dev0.close()

    def fn(dev, rank, world):
        kzg = KZG(dev, q.Srs.generate(dev, tau, L, offset=rank * L), N - 1)
        vec = q.DeviceVec.from_list(dev, poly[rank * L:(rank + 1) * L])
        t = Transcript(b"shard-check")
        c0 = dev.counter("open_checks")
        a = arm(rank) if arm else None
        if a:
            dev.debug_open_fault(*a)
        try:
            res = (kzg.open_dev(vec, L, pt, t), t.state, dev.counter("open_checks") - c0)
        except QuillGpuError as e:
            assert "Polynomial division failed" in str(e)
            res = e.code
        vec.close()
        kzg.srs.close()
        return res
    before = threading.active_count()
    out = run_ranks(world, fn)
    assert threading.active_count() == before  # no rank is stuck in a collective
    return ref, t_ref.state, out


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_check_is_silent(world):
    ref, st, out = sharded_case(world)
    for res in out:
        assert res == (ref, st, 4)


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_corrupt_quotient_on_one_rank_fails_every_rank(world):
    _, _, out = sharded_case(world, arm=lambda r: (2, 3) if r == 1 else None)
    assert out == [-5] * world


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_short_trim_on_the_top_rank_fails_every_rank(world):
    _, _, out = sharded_case(world, arm=lambda r: (1, 5) if r == world - 1 else None)
    assert out == [-5] * world


@pytest.mark.parametrize("fault", [None, (2, 1000), (1, 9)])
def test_sharded_batch(fault):
    """three items at world 2 through mle_open_batch_sharded: the single-context
    proofs, 12 checks per rank; with a fault on rank 1 both ranks fail"""
    import quill_amd as q
    from quill_amd import KZG, Transcript
    from quill_amd._lib import QuillGpuError
    from test_gpu_multirank import run_ranks
    world, nv = 2, 12
    rnd = random.Random(8800)
    tau = rnd.randrange(R)
    polys = [[rnd.randrange(1, R) for _ in range(1 << nv)] for _ in range(3)]
    pts = [[rnd.randrange(R) for _ in range(nv)] for _ in range(3)]
    dev0 = q.Device(0)
    kz = KZG.trusted_setup(1 << nv, tau, dev0)
    vs = [q.DeviceVec.from_list(dev0, p) for p in polys]
    t_ref = Transcript(b"shard-check-batch")
    ref = kz.open_batch_dev([(v, 1 << nv, pt, False) for v, pt in zip(vs, pts)], t_ref)
    for v in vs:
        v.close()
    kz.close()
    dev0.close()

    def fn(dev, rank, world):
        kzg = KZG.trusted_setup(1 << nv, tau, dev)
        L = (1 << nv) // world
        vecs = [q.DeviceVec.from_list(dev, p[rank * L:(rank + 1) * L]) for p in polys]
        t = Transcript(b"shard-check-batch")
        c0 = dev.counter("open_checks")
        if fault and rank == 1:
            dev.debug_open_fault(*fault)
        try:
            got = kzg.open_batch_dev([(v, L, pt, False) for v, pt in zip(vecs, pts)], t)
            res = (got, t.state, dev.counter("open_checks") - c0)
        except QuillGpuError as e:
            assert "Polynomial division failed" in str(e)
            res = e.code
        for v in vecs:
            v.close()
        kzg.close()
        return res
    before = threading.active_count()
    out = run_ranks(world, fn)
    assert threading.active_count() == before
    if fault:
        assert out == [-5] * world
    else:
        for res in out:
            assert res == (ref, t_ref.state, 12)
