"""Multi-tile scatter blocks of the MSM bucketing (csrc/msm.hip:
k_sortA_scatter<BLK, PF> walks the tiles k = blockIdx.x, + gridDim.x, ...,
k_sortB_scatter<BLK, CHUNK, PF> the chunks; the 1024-thread instantiations
prefetch the next tile into registers and a second LDS row buffer).  Only an
MSM of 2^26 entries takes that path by default, so the wide kernels are forced
at small sizes by QG_SORT_BLOCK_A / _TILE / _BLOCK_B / _CHUNK and the block
counts by QG_SORT_GRID_A / QG_SORT_GRID_B (0 = one block per tile).

One SRS of 2^15 bases [tau^i] g with c = 16 (16 windows, H = 128 groups, NL =
256 buckets per group): a tile of 1024 scalars fits the LDS there (with the
default c = 13 of that size it is refused, tests/test_gpu_sort_geometry.py).
Every commitment is compared with the trapdoor value [p(tau)] g; special
scalar patterns also with the CPU oracle's MSM over the downloaded bases.

Defined behaviour of the overrides, asserted below: any block count in
[0, 2^20] runs and gives the same commitment, a multiple of 8 or not (that
only decides whether a block's tiles stay in one XCD's range), also a count
above the tile count (the blocks without a tile exit before their first
barrier); anything else is QG_ERR_INVALID before a launch.

Chunk boundaries of pass B (signed 16-bit digits, bucket = digit - 1, group =
bucket >> 8, restated in digits() below):
  * scalars 1..256 have one digit each, all in group 0 of window 0: n = 16384
    fills exactly one chunk of 16384, n = 16385 is one entry past it;
  * the scalar with every 16-bit digit 0x1234 puts 16 entries per scalar into
    one bucket: n = 1024 ends that group on the chunk boundary, n = 2048 on the
    second, n = 1025 and 2049 are 16 entries past; at n = 4096 the group is
    four whole chunks, which a grid of 2 gives to one block two at a time.
"""
import contextlib
import os
import random

import pytest

import quill_oracle as o

pytestmark = pytest.mark.gpu
R = o.R_MOD
TAU = 0x50495045
LOG_N = 15
TILE = 1024
CHUNK = 16384
WIDE = dict(QG_SORT_BLOCK_A="1024", QG_SORT_TILE="1024", QG_SORT_BLOCK_B="1024",
            QG_SORT_CHUNK="16384")
ALL = tuple(WIDE) + ("QG_SORT_GRID_A", "QG_SORT_GRID_B")
N_TILES = (1 << 13) + 37          # 9 tiles, the last of 37 scalars
SAME_DIGIT = sum(0x1234 << (16 * w) for w in range(16))


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


def digits(s, c=16, W=16):
    """the kernels' signed digits of a canonical scalar: [(window, bucket)]"""
    out, carry = [], 0
    for w in range(W):
        d = ((s >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 1 if d > (1 << (c - 1)) else 0
        mag = (1 << c) - d if carry else d
        if mag:
            out.append((w, mag - 1))
    return out


def heaviest_group(scal, lo=8):
    cnt = {}
    for s in scal:
        for _w, b in digits(s):
            cnt[b >> lo] = cnt.get(b >> lo, 0) + 1
    return max(cnt.values()) if cnt else 0


def scalars(kind, n):
    rnd = random.Random("sort-pipeline-" + kind)
    if kind == "random":
        return [rnd.randrange(R) for _ in range(n)]
    if kind == "zero":
        return [0] * n
    if kind == "equal":
        return [rnd.randrange(R)] * n
    if kind == "same_digit":
        return [SAME_DIGIT] * n
    if kind == "r_minus_1":
        return [R - 1] * n
    if kind == "bits20":
        return [rnd.randrange(1 << 20) for _ in range(n)]
    assert kind == "group0"
    return [1 + rnd.randrange(256) for _ in range(n)]


_STATE = {}


@pytest.fixture(scope="module")
def srs(dev):
    from quill_amd import Srs
    with env(QG_MSM_WINDOW_BITS="16"):
        s = Srs.generate(dev, TAU, 1 << LOG_N)
    assert s.window_info() == (16, 16)
    yield s
    for k in [k for k in _STATE if k[0] == "vec"]:
        _STATE.pop(k).close()
    _STATE.clear()
    s.close()


def case(dev, kind):
    """device vector of the pattern (2^15 scalars), the scalars, and
    expected(n) = [p(tau)] g of the first n"""
    from quill_amd import DeviceVec
    if ("vec", kind) not in _STATE:
        scal = scalars(kind, 1 << LOG_N)
        _STATE["vec", kind] = DeviceVec.from_list(dev, scal)
        _STATE["scal", kind] = scal
        _STATE["want", kind] = {}
    want = _STATE["want", kind]

    def expected(n):
        if n not in want:
            want[n] = o.g1_mul(o.G1_GEN, o.poly_eval(_STATE["scal", kind][:n], TAU))
        return want[n]
    return _STATE["vec", kind], _STATE["scal", kind], expected


def cpu_msm(srs, scal, n):
    import oracle_c as oc
    if "bases" not in _STATE:
        _STATE["bases"] = srs.download(0, 1 << 12)
    return oc.msm(_STATE["bases"][:n], scal[:n])


def run(srs, vec, n, grid_a, grid_b):
    with env(**WIDE), env(QG_SORT_GRID_A=str(grid_a), QG_SORT_GRID_B=str(grid_b)):
        return srs.msm_dev(vec, n)


def plain(srs, vec, n):
    with env(**{k: None for k in ALL}):
        return srs.msm_dev(vec, n)


@pytest.mark.parametrize("grid", [1, 2, 3, 8, 9, 0, 16, 1024])
def test_tiles_per_block(dev, srs, grid):
    """9 tiles (the last partial) and ~128 chunks over 1 / 2 / 3 / 8 blocks
    (one block walks everything; unequal shares; not a multiple of 8), one block
    per tile (9 = the tile count, and 0), and more blocks than tiles"""
    vec, _scal, expected = case(dev, "random")
    want = expected(N_TILES)
    assert plain(srs, vec, N_TILES) == want
    assert run(srs, vec, N_TILES, grid, grid) == want
    # the two passes independently: the other one block per tile / chunk
    assert run(srs, vec, N_TILES, grid, 0) == want
    assert run(srs, vec, N_TILES, 0, grid) == want


@pytest.mark.parametrize("grid", [2, 8])
@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, 6 * TILE + 1, 7 * TILE, 9 * TILE,
                               17 * TILE - 3])
def test_lengths(dev, srs, n, grid):
    """one scalar; around one tile; 7, 9 and 17 tiles (xcd_tile's remainder
    ranges: 7 = 0 x 8 + 7, 9 = 8 + 1, 17 = 2 x 8 + 1)"""
    vec, _scal, expected = case(dev, "random")
    want = expected(n)
    assert run(srs, vec, n, grid, grid) == want
    assert plain(srs, vec, n) == want


@pytest.mark.parametrize("kind", ["zero", "equal", "same_digit", "r_minus_1", "bits20", "random"])
def test_scalar_patterns(dev, srs, kind):
    n = 1 << 12
    vec, scal, expected = case(dev, kind)
    want = expected(n)
    if kind == "zero":
        assert want is None
    if kind == "same_digit":  # one bucket holds everything: four whole chunks
        assert heaviest_group(scal[:n]) == 4 * CHUNK
    if kind == "bits20":
        assert all(w <= 1 for s in scal[:n] for w, _b in digits(s))
    got = run(srs, vec, n, 2, 2)
    assert got == want
    if kind != "random":
        assert got == cpu_msm(srs, scal, n)
    assert run(srs, vec, n, 1, 1) == want
    assert plain(srs, vec, n) == want


@pytest.mark.parametrize("grid", [2, 0])
@pytest.mark.parametrize("kind,n,entries", [
    ("group0", CHUNK, CHUNK), ("group0", CHUNK + 1, CHUNK + 1),
    ("same_digit", 1024, CHUNK), ("same_digit", 1025, CHUNK + 16),
    ("same_digit", 2048, 2 * CHUNK), ("same_digit", 2049, 2 * CHUNK + 16),
])
def test_chunk_boundaries(dev, srs, kind, n, entries, grid):
    """the heaviest group ends on a chunk boundary of pass B, or just past it"""
    vec, scal, expected = case(dev, kind)
    assert heaviest_group(scal[:n]) == entries
    want = expected(n)
    assert run(srs, vec, n, grid, grid) == want
    assert plain(srs, vec, n) == want


@pytest.mark.parametrize("bad", ["-1", str((1 << 20) + 1), "many", "8x", ""])
@pytest.mark.parametrize("which", ["QG_SORT_GRID_A", "QG_SORT_GRID_B"])
def test_grid_out_of_range_is_rejected(dev, srs, which, bad):
    from quill_amd._lib import QuillGpuError
    vec, _scal, expected = case(dev, "random")
    n = 1027
    dev.enable_timing(True)
    try:
        before = dev.kernel_time("msm_bucketing")[1]
        with env(**{k: None for k in ALL}), env(**WIDE), env(**{which: bad}):
            with pytest.raises(QuillGpuError) as ei:
                srs.msm_dev(vec, n)
        assert ei.value.code == -1  # QG_ERR_INVALID
        assert dev.kernel_time("msm_bucketing")[1] == before  # nothing was launched
        assert plain(srs, vec, n) == expected(n)
    finally:
        dev.enable_timing(False)


def test_one_iteration_paths(dev, srs):
    """the default grids outside the wide class (one block per tile): a batch
    on the side streams and a one-shot table equal the same MSMs run singly"""
    from quill_amd import DeviceVec, Srs
    n = 1 << 12
    vecs, wants = [], []
    for i in range(3):
        rnd = random.Random("sort-pipeline-batch-%d" % i)
        scal = [rnd.randrange(R) for _ in range(n)]
        vecs.append(DeviceVec.from_list(dev, scal))
        wants.append(o.g1_mul(o.G1_GEN, o.poly_eval(scal, TAU)))
    try:
        with env(**{k: None for k in ALL}):
            single = [srs.msm_dev(v, n) for v in vecs]
            assert single == wants
            assert srs.msm_dev_batch(vecs) == single
            xy, inf = srs.download_raw(0, n)
            one = Srs.upload_raw(dev, xy, inf, oneshot=True)
            try:
                assert [one.msm_dev(v, n) for v in vecs] == single
                assert one.msm_dev_batch(vecs) == single
            finally:
                one.close()
    finally:
        for v in vecs:
            v.close()
