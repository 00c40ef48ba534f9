"""The launch geometries of the MSM bucketing's sort kernels (csrc/msm.hip:
k_sortA_rows / k_sortA_scatter<BLK> over a tile of scalars, k_sortB_hist /
k_sortB_scatter<BLK, CHUNK> over a chunk of entries).  Every instantiated
pass-A geometry x every pass-B geometry is forced by QG_SORT_BLOCK_A /
QG_SORT_TILE / QG_SORT_BLOCK_B / QG_SORT_CHUNK; each MSM must equal the
trapdoor value [p(tau)] g and the default geometry's result.

  * two SRS of 2^15 bases: c = 20 (H = 512 groups, NL = 1024 buckets per group,
    the 2^24 headline's split) and the default c of that size (c = 13, H = NL =
    64: lds_exscan with fewer counts than threads).  With the default c's 20
    windows a tile of 1024 scalars does not fit the LDS (the library refuses
    it, asserted here), so a third SRS with c = 16 (16 windows, H = 128,
    NL = 256) runs the tile-1024 geometries with few counts;
  * lengths 1, tile - 1, tile, tile + 1, 2 tile + 3 and 20 011: partial tiles,
    partial last waves, n no multiple of the block;
  * scalars: full-width random; all equal to one random value (13 buckets of n
    entries: at n = 20 011 a group spans two chunks of 16384 and three of 8192,
    the only small input that runs cbase / chunk_group / coff across chunks);
    12-bit (window 0 only, crowded buckets); all zero (no entries, the point at
    infinity); signed-digit edges (r - 1, 2^19, 2^19 + 1, 2^20 - 1, 2^20, and
    values whose every 20-bit digit is 2^19 or 2^19 + 1: the carry runs through
    all 13 windows);
  * an override that names a geometry without an instantiation is
    QG_ERR_INVALID before anything is launched; a side-stream batch that
    fails this way returns the hand-over event it took (the context's
    events in use, `events_created` - `events_pooled`, stay as they were).
"""
import contextlib
import os
import random

import pytest

import quill_oracle as o

pytestmark = pytest.mark.gpu
R = o.R_MOD
TAU = 0x5EED50B7
LOG_N = 15
N_MAX = 20011

GEOM_A = [(256, 512), (512, 512), (512, 1024), (1024, 1024)]       # (BLK_A, tile)
GEOM_B = [(256, 8192), (512, 8192), (512, 16384), (1024, 16384)]   # (BLK_B, chunk)
KINDS = ["random", "equal", "bits12", "zero", "edges"]
OVERRIDES = ("QG_SORT_BLOCK_A", "QG_SORT_TILE", "QG_SORT_BLOCK_B", "QG_SORT_CHUNK")


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def lengths(tile):
    return [1, tile - 1, tile, tile + 1, 2 * tile + 3, N_MAX]


def scalars(kind):
    rnd = random.Random("sort-geometry-" + kind)
    if kind == "random":
        return [rnd.randrange(R) for _ in range(N_MAX)]
    if kind == "equal":
        return [rnd.randrange(R)] * N_MAX
    if kind == "bits12":
        return [rnd.randrange(1 << 12) for _ in range(N_MAX)]
    if kind == "zero":
        return [0] * N_MAX
    assert kind == "edges"
    half = 1 << 19
    pat = [R - 1, half, half + 1, (1 << 20) - 1, 1 << 20]
    for top in (0, 0x1fff):  # window 12 holds bits 240..253: r >> 240 = 0x3064
        for _ in range(6):
            v = top << 240
            for w in range(12):
                v |= (half + rnd.randrange(2)) << (20 * w)
            assert v < R
            pat.append(v)
    return [pat[i % len(pat)] for i in range(N_MAX)]


_STATE = {}


@pytest.fixture(scope="module")
def srs_of(dev):
    """kind -> SRS of 2^15 bases [tau^i] g: 'c20' / 'c16' created with 20- /
    16-bit windows, 'default' with the window bits of its size"""
    from quill_amd import Srs

    def get(kind):
        if ("srs", kind) not in _STATE:
            with env(QG_MSM_WINDOW_BITS=kind[1:] if kind != "default" else None):
                _STATE["srs", kind] = Srs.generate(dev, TAU, 1 << LOG_N)
        return _STATE["srs", kind]
    yield get
    for k in [k for k in _STATE if k[0] in ("srs", "vec")]:
        _STATE.pop(k).close()
    _STATE.clear()


def case(dev, kind):
    """the scalar vector on the device and {n: trapdoor value of its first n}"""
    from quill_amd import DeviceVec
    if ("vec", kind) not in _STATE:
        scal = scalars(kind)
        _STATE["vec", kind] = DeviceVec.from_list(dev, scal)
        _STATE["scal", kind] = scal
        _STATE["want", kind] = {}
    want = _STATE["want", kind]

    def expected(n):
        if n not in want:
            want[n] = o.g1_mul(o.G1_GEN, o.poly_eval(_STATE["scal", kind][:n], TAU))
        return want[n]
    return _STATE["vec", kind], expected


def default_result(srs_kind, kind, srs, vec, n):
    key = ("default", srs_kind, kind, n)
    if key not in _STATE:
        with env(**{k: None for k in OVERRIDES}):
            _STATE[key] = (srs.msm_dev(vec, n),)
    return _STATE[key][0]


def test_window_sets(srs_of):
    c, W = srs_of("c20").window_info()
    assert (c, W) == (20, 13)  # H = 512, NL = 1024
    assert srs_of("c16").window_info() == (16, 16)  # H = 128, NL = 256
    c, W = srs_of("default").window_info()
    assert c - 1 <= 16  # H, NL <= 256: fewer counts than the narrowest block has threads


@pytest.mark.parametrize("geom_a", GEOM_A, ids=lambda g: "A%dx%d" % g)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("srs_kind", ["c20", "default", "c16"])
def test_every_geometry(dev, srs_of, srs_kind, kind, geom_a):
    from quill_amd._lib import QuillGpuError
    srs = srs_of(srs_kind)
    vec, expected = case(dev, kind)
    blk_a, tile = geom_a
    # a tile's staged digits (8 B each, W per scalar) must fit the CU's 160 KiB
    # of LDS: the default c of 2^15 bases is 13 with W = 20 windows, where a
    # tile of 1024 cannot run at any block width and is refused before a launch
    if tile * srs.window_info()[1] * 8 >= 160 * 1024:
        assert srs_kind == "default" and tile == 1024
        for blk_b, chunk in GEOM_B:
            with env(QG_SORT_BLOCK_A=str(blk_a), QG_SORT_TILE=str(tile),
                     QG_SORT_BLOCK_B=str(blk_b), QG_SORT_CHUNK=str(chunk)):
                with pytest.raises(QuillGpuError) as ei:
                    srs.msm_dev(vec, N_MAX)
            assert ei.value.code == -4  # QG_ERR_UNSUPPORTED
        assert default_result(srs_kind, kind, srs, vec, N_MAX) == expected(N_MAX)
        return
    for n in lengths(tile):
        want = expected(n)
        if kind == "zero":
            assert want is None
        base = default_result(srs_kind, kind, srs, vec, n)
        assert base == want, (n, "default geometry")
        for blk_b, chunk in GEOM_B:
            with env(QG_SORT_BLOCK_A=str(blk_a), QG_SORT_TILE=str(tile),
                     QG_SORT_BLOCK_B=str(blk_b), QG_SORT_CHUNK=str(chunk)):
                got = srs.msm_dev(vec, n)
            assert got == want, (n, geom_a, blk_b, chunk)
            assert got == base, (n, geom_a, blk_b, chunk)


@pytest.mark.parametrize("bad", [
    dict(QG_SORT_BLOCK_A="384"),
    dict(QG_SORT_BLOCK_A="128"),
    dict(QG_SORT_BLOCK_A="2048", QG_SORT_TILE="1024"),
    dict(QG_SORT_BLOCK_A="1024", QG_SORT_TILE="512"),
    dict(QG_SORT_BLOCK_A="512", QG_SORT_TILE="256"),
    dict(QG_SORT_TILE="768"),
    dict(QG_SORT_BLOCK_B="256", QG_SORT_CHUNK="16384"),
    dict(QG_SORT_BLOCK_B="1024", QG_SORT_CHUNK="8192"),
    dict(QG_SORT_BLOCK_B="512", QG_SORT_CHUNK="4096"),
    dict(QG_SORT_CHUNK="0"),
    dict(QG_SORT_BLOCK_B="64"),
], ids=lambda d: ",".join("%s=%s" % (k[8:], v) for k, v in d.items()))
def test_geometry_without_instantiation_is_rejected(dev, srs_of, bad):
    from quill_amd._lib import QuillGpuError
    srs = srs_of("c20")
    vec, expected = case(dev, "random")
    n = 1027
    dev.enable_timing(True)
    try:
        before = dev.kernel_time("msm_bucketing")[1]
        with env(**{k: None for k in OVERRIDES}), env(**bad):
            with pytest.raises(QuillGpuError) as ei:
                srs.msm_dev(vec, n)
        assert ei.value.code == -1  # QG_ERR_INVALID
        assert dev.kernel_time("msm_bucketing")[1] == before  # nothing was launched
        # the context is unharmed: the same MSM with the default geometry
        assert default_result("c20", "random", srs, vec, n) == expected(n)
    finally:
        dev.enable_timing(False)


def test_failing_batch_returns_its_events(dev, srs_of):
    """A side-stream batch that fails after it took its first hand-over event
    (the bad geometry is found when the batch sizes its scratch) hands the
    event back: the events in use (created - pooled; the session's context
    has a well-filled pool, so `events_created` alone would not move) are as
    many after every failing batch as before, repeating it creates no further
    event, and the same batch without the override is correct."""
    from quill_amd._lib import QuillGpuError
    srs = srs_of("c20")
    vec, expected = case(dev, "random")
    ns = [1027, 513]

    def failing_batch():
        with env(**{k: None for k in OVERRIDES}), env(QG_SORT_BLOCK_A="384", QG_MSM_PIPE=None):
            with pytest.raises(QuillGpuError) as ei:
                srs.msm_dev_batch([vec, vec], ns)
        assert ei.value.code == -1  # QG_ERR_INVALID

    def in_use():
        return dev.counter("events_created") - dev.counter("events_pooled")

    before = in_use()
    failing_batch()
    assert in_use() == before
    created = dev.counter("events_created")
    for _ in range(3):
        failing_batch()
        assert in_use() == before
    assert dev.counter("events_created") == created
    with env(**{k: None for k in OVERRIDES}), env(QG_MSM_PIPE=None):
        assert srs.msm_dev_batch([vec, vec], ns) == [expected(n) for n in ns]
