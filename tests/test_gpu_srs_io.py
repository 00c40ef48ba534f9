"""SRS import / export as ark-serialize bytes, decoded and validated on the
device (qg_srs_import, qg_srs_export, qg_srs_validate): imports equal
qg_srs_upload of the same points bit for bit, exports equal the host
serializer and the Python restatement, every malformed encoding is refused
with its exact index and reason, and qg_srs_validate finds an off-curve point
that qg_srs_upload took."""
import ctypes as C

import numpy as np
import pytest

import quill_oracle as o
import srs_bytes_restatement as sb

pytestmark = pytest.mark.gpu
P = o.P_MOD
NMAX = 4097
INF_AT = 3  # the infinity point of every point set longer than this


@pytest.fixture(scope="module")
def base(dev):
    """NMAX points [tau^i] g from a generated SRS with one infinity point:
    (points, ABI limbs, infinity flags); shared, never modified"""
    from quill_amd import Srs
    gen = Srs.generate(dev, 0x535253494F, NMAX)
    xy, inf = gen.download_raw()
    gen.close()
    xy, inf = xy.copy(), inf.copy()
    xy[INF_AT, :] = 0
    inf[INF_AT] = 1
    from quill_amd.field import g1_from_abi
    pts = [g1_from_abi(xy[i], inf[i]) for i in range(NMAX)]
    assert {sb.is_larger(p[1]) for p in pts[:255] if p} == {True, False}  # both signs
    xy.setflags(write=False)
    inf.setflags(write=False)
    return pts, xy, inf


def _same_tables(dev, a, b, n, seed):
    """download(), an MSM of random scalars and the window geometry agree"""
    import quill_amd as q
    axy, ainf = a.download_raw()
    bxy, binf = b.download_raw()
    assert np.array_equal(ainf, binf) and np.array_equal(axy, bxy)
    assert a.window_info() == b.window_info()
    v = q.DeviceVec(dev, n).fill_random(seed)
    assert a.msm_dev(v, n) == b.msm_dev(v, n)
    v.close()


@pytest.mark.parametrize("compressed", [False, True])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097])
def test_import_equals_upload(dev, base, n, compressed):
    from quill_amd import Srs
    pts, xy, inf = base
    up = Srs.upload_raw(dev, xy[:n], inf[:n])
    imp = Srs.from_bytes(dev, sb.ser_points(pts[:n], compressed), compressed)
    assert len(imp) == n
    _same_tables(dev, imp, up, n, 7000 + n)
    imp.validate()
    imp.close()
    up.close()


@pytest.mark.parametrize("compressed", [False, True])
def test_import_oneshot_equals_bases_upload(dev, base, compressed):
    from quill_amd import Srs
    pts, xy, inf = base
    up = Srs.upload_raw(dev, xy, inf, oneshot=True)
    imp = Srs.from_bytes(dev, sb.ser_points(pts, compressed), compressed, oneshot=True)
    _same_tables(dev, imp, up, NMAX, 7100)
    imp.close()
    up.close()


def _edge_xs():
    """the largest x below p and the smallest above 0 with a square x^3 + 3"""
    hi = next(x for x in range(P - 1, 0, -1) if sb.fq_sqrt((x * x * x + 3) % P) is not None)
    lo = next(x for x in range(1, P) if sb.fq_sqrt((x * x * x + 3) % P) is not None)
    return lo, hi


def test_decode_operand_edges(dev):
    """the generator and the extreme x coordinates, both roots through the sign
    flag, compressed and uncompressed"""
    from quill_amd import Srs
    lo, hi = _edge_xs()
    assert lo == 1  # the generator's x
    pts = []
    for x in (1, lo, hi):
        y = sb.fq_sqrt((x * x * x + 3) % P)
        small, large = min(y, P - y), max(y, P - y)
        pts += [(x, small), (x, large)]
    assert o.G1_GEN in pts
    for compressed in (True, False):
        data = sb.ser_points(pts, compressed)
        srs = Srs.from_bytes(dev, data, compressed)
        assert srs.download() == pts
        assert srs.to_bytes(compressed=compressed) == data
        srs.close()
    # the sign flag alone selects the root of a compressed point
    for i, (x, y) in enumerate(pts):
        b = bytearray(x.to_bytes(32, "little"))
        b[31] |= sb.NEG if i % 2 else 0
        srs = Srs.from_bytes(dev, bytes(b), True)
        assert srs.download() == [(x, y)]
        srs.close()


def test_export_equals_host_serializer_and_restatement(dev, base):
    from quill_amd import Srs, lib
    pts, xy, inf = base
    n = 300
    srs = Srs.upload_raw(dev, xy[:n], inf[:n])
    dxy, dinf = srs.download_raw()
    host = bytearray()
    for i in range(n):
        out = (C.c_uint8 * 64)()
        row = np.ascontiguousarray(dxy[i])
        assert lib().qg_g1_serialize(row.ctypes.data_as(C.POINTER(C.c_uint64)), int(dinf[i]),
                                     out) == 0
        host += bytes(out)
    assert srs.to_bytes(compressed=False) == bytes(host) == sb.ser_points(pts[:n], False)
    assert srs.to_bytes(compressed=True) == sb.ser_points(pts[:n], True)
    for off, m in ((0, 1), (1, 255), (INF_AT, 1), (44, 256), (299, 1), (300, 0)):
        for c in (False, True):
            assert srs.to_bytes(off, m, c) == sb.ser_points(pts[off:off + m], c)
    from quill_amd import QuillGpuError
    with pytest.raises(QuillGpuError):
        srs.to_bytes(299, 2)
    srs.close()


@pytest.mark.parametrize("compressed", [False, True])
def test_bytes_round_trip(dev, base, compressed):
    from quill_amd import Srs
    pts, xy, inf = base
    n = 513
    up = Srs.upload_raw(dev, xy[:n], inf[:n])
    data = up.to_bytes(compressed=compressed)
    again = Srs.from_bytes(dev, data, compressed)
    _same_tables(dev, again, up, n, 7200)
    assert again.to_bytes(compressed=compressed) == data
    # a sub-range of the bytes, without a copy on the caller's side
    part = Srs.from_bytes(dev, memoryview(data), compressed, offset=100, n=257)
    assert part.download() == pts[100:357]
    part.close()
    again.close()
    up.close()


def _le(v):
    return v.to_bytes(32, "little")


def _bad_cases():
    x, y = o.g1_mul(o.G1_GEN, 1234567)
    gu, gc = sb.ser_g1_uncompressed((x, y)), sb.ser_g1_compressed((x, y))
    inf_x = bytearray(32)
    inf_x[0], inf_x[31] = 1, sb.INF
    inf_y = bytearray(64)
    inf_y[40], inf_y[63] = 1, sb.INF
    flip_y = bytearray(gu)
    flip_y[35] ^= 4
    flip_sign = bytearray(gu)
    flip_sign[63] ^= sb.NEG
    cases = []
    for name, v in (("x=p", P), ("x=p+1", P + 1), ("x=2^254-1", (1 << 254) - 1)):
        cases.append((name + " compressed", True, _le(v), sb.NONCANONICAL))
        cases.append((name + " uncompressed", False, _le(v) + gu[32:], sb.NONCANONICAL))
    cases += [
        ("y=p", False, gu[:32] + _le(P), sb.NONCANONICAL),
        ("zeros compressed", True, bytes(32), sb.NOT_SQUARE),
        ("zeros uncompressed", False, bytes(64), sb.NOT_ON_CURVE),
        ("x=4", True, _le(4), sb.NOT_SQUARE),
        ("inf+x compressed", True, bytes(inf_x), sb.BAD_INFINITY),
        ("inf+sign compressed", True, bytes(31) + bytes([sb.INF | sb.NEG]), sb.BAD_INFINITY),
        ("inf+y uncompressed", False, bytes(inf_y), sb.BAD_INFINITY),
        ("inf+sign uncompressed", False, bytes(63) + bytes([sb.INF | sb.NEG]), sb.BAD_INFINITY),
        ("bit of y", False, bytes(flip_y), sb.NOT_ON_CURVE),
        ("sign flag", False, bytes(flip_sign), sb.SIGN_FLAG),
    ]
    return cases


BAD = _bad_cases()


def _good_commit(dev, base):
    """after a refusal the context still imports and commits correctly"""
    from quill_amd import Srs
    pts, xy, inf = base
    n = 64
    good = Srs.from_bytes(dev, sb.ser_points(pts[:n], True), True)
    up = Srs.upload_raw(dev, xy[:n], inf[:n])
    sc = [(i * 0x9E3779B97F4A7C15 + 1) % o.R_MOD for i in range(n)]
    assert good.msm(sc) == up.msm(sc)
    good.close()
    up.close()


@pytest.mark.parametrize("case", range(len(BAD)), ids=[c[0] for c in BAD])
def test_rejections(dev, base, case):
    from quill_amd import QuillGpuError, Srs
    pts, _, _ = base
    name, compressed, enc, reason = BAD[case]
    # the restatement refuses it for the same reason
    with pytest.raises(sb.BadPoint) as e:
        (sb.de_g1_compressed if compressed else sb.de_g1_uncompressed)(enc)
    assert e.value.reason == reason
    pb = len(enc)
    for n, at in ((9, 5), (1, 0), (300, 299)):
        data = bytearray(sb.ser_points(pts[:n], compressed))
        data[at * pb:(at + 1) * pb] = enc
        with pytest.raises(QuillGpuError) as e:
            Srs.from_bytes(dev, bytes(data), compressed)
        assert (e.value.code, e.value.bad_index, e.value.bad_reason) == (-1, at, reason), name
        assert f"point {at}" in str(e.value) and f"reason {reason}" in str(e.value)
    _good_commit(dev, base)


@pytest.mark.parametrize("compressed", [False, True])
def test_lowest_bad_index_is_reported_every_time(dev, base, compressed):
    from quill_amd import QuillGpuError, Srs
    pts, _, _ = base
    pb = 32 if compressed else 64
    data = bytearray(sb.ser_points(pts, compressed))
    hi_bad = _le(4) if compressed else bytes(64)            # reasons 3 / 4
    lo_bad = _le(P) + (b"" if compressed else bytes(32))    # reason 1
    data[300 * pb:301 * pb] = hi_bad
    data[7 * pb:8 * pb] = lo_bad
    data = bytes(data)
    for _ in range(3):
        with pytest.raises(QuillGpuError) as e:
            Srs.from_bytes(dev, data, compressed)
        assert (e.value.bad_index, e.value.bad_reason) == (7, sb.NONCANONICAL)
    _good_commit(dev, base)


def test_import_argument_errors(dev):
    from quill_amd import QuillGpuError, Srs, lib
    with pytest.raises(QuillGpuError):
        Srs.from_bytes(dev, bytes(33), True)
    h = C.c_void_p()
    buf = C.create_string_buffer(64)
    L = lib()
    assert L.qg_srs_import(dev.h, buf, 1, 2, 0, C.byref(h), None, None) == -1  # format
    assert L.qg_srs_import(dev.h, buf, 1, 1, 2, C.byref(h), None, None) == -1  # flags
    assert L.qg_srs_import(dev.h, buf, 0, 1, 0, C.byref(h), None, None) == -1  # empty
    assert L.qg_srs_import(dev.h, buf, 1 << 62, 0, 0, C.byref(h), None, None) == -1
    assert L.qg_srs_import(None, buf, 1, 1, 0, C.byref(h), None, None) == -1
    assert not h.value


def test_validate_accepts_generated_and_uploaded(dev, base):
    from quill_amd import Srs
    _, xy, inf = base
    gen = Srs.generate(dev, 31337, 1000)
    gen.validate()
    gen.close()
    for oneshot in (False, True):
        up = Srs.upload_raw(dev, xy[:600], inf[:600], oneshot)
        up.validate()
        up.close()


@pytest.mark.parametrize("at", [0, 255, 256, 598])
def test_validate_names_the_off_curve_point_upload_took(dev, base, at):
    """qg_srs_upload checks nothing: a point with a wrong y loads; validate
    names it (and the lower of two)"""
    from quill_amd import QuillGpuError, Srs
    from quill_amd.field import g1_to_abi
    pts, xy, inf = base
    n = 600
    bad = xy[:n].copy()
    for k in (at, 599):
        x, y = pts[k]
        assert not o.g1_is_on_curve((x, (y + 1) % P))
        bad[k, :] = list(g1_to_abi((x, (y + 1) % P))[0])
    srs = Srs.upload_raw(dev, bad, inf[:n])  # accepted
    for _ in range(2):
        with pytest.raises(QuillGpuError) as e:
            srs.validate()
        assert (e.value.code, e.value.bad_index, e.value.bad_reason) == (-1, at, sb.NOT_ON_CURVE)
    srs.close()
