"""qg_srs_check_powers: is an SRS [tau^i] g1 for the tau of the verifier's
tau g2?  One random linear combination (multipliers from BLAKE3 on the device,
two MSMs, two host Miller loops), single-context and sharded over loopback
ranks, and KZG.from_bytes on a sharded device (an imported SRS with no tau)."""
import random
import threading

import numpy as np
import pytest

import quill_oracle as o
import srs_bytes_restatement as sb
from test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu
R = o.R_MOD
TAU = 0x706F77657273206F662074617500000000001234567
SEEDS = (bytes(range(32)), bytes([0xA5]) * 32)


@pytest.fixture(scope="module")
def g2pts():
    import quill_amd as q
    g2 = q.g2_generator()
    return [g2, q.g2_mul(g2, TAU)]


@pytest.fixture(scope="module")
def raw257(dev):
    """a generated 257-point SRS as ABI limbs (never modified)"""
    from quill_amd import Srs
    s = Srs.generate(dev, TAU, 257)
    xy, inf = s.download_raw()
    s.close()
    xy.setflags(write=False)
    return xy, inf


@pytest.mark.parametrize("N", [1, 2, 3, 257, 4097])
def test_accepts_generated(dev, g2pts, N):
    from quill_amd import Srs
    s = Srs.generate(dev, TAU, N)
    assert s.check_powers(o.G1_GEN, g2pts) is True  # a fresh random seed
    assert s.check_powers(o.G1_GEN, g2pts, SEEDS[0]) is True
    s.close()


def test_accepts_second_generator_and_rejects_wrong_g1(dev, g2pts):
    from quill_amd import Srs
    g = o.g1_mul(o.G1_GEN, 5)
    s = Srs.generate(dev, TAU, 300, g=g)
    for seed in SEEDS:
        assert s.check_powers(g, g2pts, seed) is True
        # every link holds, but the first point is not vk.g1
        assert s.check_powers(o.G1_GEN, g2pts, seed) is False
    one = Srs.generate(dev, TAU, 1, g=g)
    assert one.check_powers(g, g2pts) is True and one.check_powers(o.G1_GEN, g2pts) is False
    one.close()
    s.close()


def _corrupt(xy, kind):
    xy = xy.copy()
    if kind == "swap":      # two interior points swapped (a constant rho would pass)
        xy[[100, 101]] = xy[[101, 100]]
    elif kind == "replace":  # another valid curve point
        xy[50] = xy[7]
    elif kind == "last":
        xy[256] = xy[3]
    return xy


@pytest.mark.parametrize("kind", ["swap", "replace", "last"])
def test_rejects_corrupted(dev, g2pts, raw257, kind):
    from quill_amd import Srs
    xy, inf = raw257
    s = Srs.upload_raw(dev, _corrupt(xy, kind), inf)
    s.validate()  # every point is on the curve: only the powers check sees it
    for seed in SEEDS:
        assert s.check_powers(o.G1_GEN, g2pts, seed) is False
    assert s.check_powers(o.G1_GEN, g2pts) is False
    s.close()


def test_rejects_other_tau(dev, raw257):
    import quill_amd as q
    from quill_amd import Srs
    xy, inf = raw257
    g2 = q.g2_generator()
    s = Srs.upload_raw(dev, xy, inf)
    for seed in SEEDS:
        assert s.check_powers(o.G1_GEN, [g2, q.g2_mul(g2, TAU)], seed) is True
        assert s.check_powers(o.G1_GEN, [g2, q.g2_mul(g2, TAU + 1)], seed) is False
    s.close()


def test_rho_matches_restatement(dev, g2pts):
    """a 2-point SRS (g, k g) passes only for k = tau, and the A, B that the
    restatement builds from rho(seed, i) reach the same verdict"""
    from quill_amd import Srs
    seed = SEEDS[1]
    for k in (TAU, TAU + 1, 1):
        pts = [o.G1_GEN, o.g1_mul(o.G1_GEN, k)]
        s = Srs.upload(dev, pts)
        got = s.check_powers(o.G1_GEN, g2pts, seed)
        A, B = sb.powers_sums(pts, seed)
        assert A == o.g1_mul(o.G1_GEN, sb.rho(seed, 0))
        assert got is (o.g1_mul(A, TAU) == B) is (k == TAU)
        s.close()


def test_multipliers_are_the_restatements(dev, g2pts):
    """the device multipliers themselves: (g, a g, b g) with a != tau passes
    exactly when rho_0 (tau - a) + rho_1 (tau a - b) == 0, so a b built from the
    restatement's rho(seed, 0) / rho(seed, 1) passes under that seed alone"""
    from quill_amd import Srs
    seed, other = SEEDS
    a = TAU + 12345
    r0, r1 = sb.rho(seed, 0), sb.rho(seed, 1)
    b = (TAU * a + r0 * (TAU - a) * pow(r1, R - 2, R)) % R
    s = Srs.upload(dev, [o.G1_GEN, o.g1_mul(o.G1_GEN, a), o.g1_mul(o.G1_GEN, b)])
    assert s.check_powers(o.G1_GEN, g2pts, seed) is True
    assert s.check_powers(o.G1_GEN, g2pts, other) is False
    assert s.check_powers(o.G1_GEN, g2pts) is False
    s.close()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded(world, g2pts):
    """64 points per rank: accepted on every rank; a corrupted point at a shard
    boundary (rank 1's first, rank 0's last) is rejected on EVERY rank"""
    import quill_amd as q
    L = 64

    def fn(dev, rank, world):
        s = q.Srs.generate(dev, TAU, L, offset=rank * L)
        xy, inf = s.download_raw()
        res = [s.check_powers(o.G1_GEN, g2pts), s.check_powers(o.G1_GEN, g2pts, SEEDS[0])]
        for bad_rank, at in ((1, 0), (0, L - 1)):
            bad = xy.copy()
            if rank == bad_rank:
                bad[at] = xy[5]
            t = q.Srs.upload_raw(dev, bad, inf)
            res += [t.check_powers(o.G1_GEN, g2pts, seed) for seed in SEEDS]
            t.close()
        # the first global point against another g1 (rank 0's verdict, shared)
        res.append(s.check_powers(o.g1_mul(o.G1_GEN, 2), g2pts, SEEDS[0]))
        s.close()
        return res
    before = threading.active_count()
    out = run_ranks(world, fn)
    assert threading.active_count() == before  # no rank is stuck in a collective
    for res in out:
        assert res == [True, True, False, False, False, False, False]


def test_kzg_from_bytes_sharded_opening_equals_trusted_setup(g2pts):
    """world 2: an ML opening over an imported SRS (bytes in an np.memmap-like
    buffer, no tau) equals the opening over KZG.trusted_setup bit for bit"""
    import quill_amd as q
    from quill_amd import KZG, Transcript
    rnd = random.Random(77)
    nv, world = 8, 2
    N = 1 << nv
    L = N // world
    poly = [rnd.randrange(R) for _ in range(N)]
    point = [rnd.randrange(R) for _ in range(nv)]
    dev0 = q.Device(0)
    full = q.Srs.generate(dev0, TAU, N)
    data = np.frombuffer(full.to_bytes(compressed=True), dtype=np.uint8)
    full.close()
    dev0.close()

    def fn(dev, rank, world):
        out = []
        for kzg in (KZG.trusted_setup(N - 1, TAU, dev),
                    KZG.from_bytes(data, g2pts, dev, compressed=True, check=True)):
            vec = q.DeviceVec.from_list(dev, poly[rank * L:(rank + 1) * L])
            t = Transcript(b"imported-srs")
            pr = kzg.open_dev(vec, L, point, t)
            out.append((pr, t.state, kzg.commit(vec)))
            vec.close()
            kzg.close()
        return out
    before = threading.active_count()
    res = run_ranks(world, fn)
    assert threading.active_count() == before
    for ref, imp in res:
        assert imp == ref
    assert res[0] == res[1]
    # the verifier accepts the opening against the imported key
    pr, _, comm = res[0][1]
    ver = KZG.verifier(g1=o.G1_GEN, g2_points=g2pts)
    assert ver.verify(comm, pr, Transcript(b"imported-srs"))


def test_kzg_from_bytes_single_device(dev, g2pts):
    import quill_amd as q
    from quill_amd import KZG, QuillGpuError
    s = q.Srs.generate(dev, TAU, 130)
    good = s.to_bytes(compressed=False)
    s.close()
    prefixed = (130).to_bytes(8, "little") + good  # an ark Vec<G1Affine>
    for data in (good, prefixed):
        kzg = KZG.from_bytes(data, g2pts, dev, compressed=False)
        assert kzg.max_degree() == 129 and kzg.g1 == o.G1_GEN
        sc = [3, 1, 4, 1, 5]
        assert kzg.commit(sc) == o.g1_mul(o.G1_GEN, o.poly_eval(sc, TAU))
        kzg.close()
    bad = bytearray(good)
    bad[64 * 9:64 * 10], bad[64 * 10:64 * 11] = good[64 * 10:64 * 11], good[64 * 9:64 * 10]
    with pytest.raises(QuillGpuError) as e:
        KZG.from_bytes(bytes(bad), g2pts, dev, compressed=False)
    assert e.value.code == -5
    kzg = KZG.from_bytes(bytes(bad), g2pts, dev, compressed=False, check=False)
    kzg.close()
