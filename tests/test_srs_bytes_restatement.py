"""The Python restatement of the SRS byte formats (tests/srs_bytes_restatement.py)
against the oracle's serializer and against itself: what the GPU tests of the
import / export compare the device with.  No GPU."""
import random

import pytest

import quill_oracle as o
import srs_bytes_restatement as sb

P = o.P_MOD


@pytest.fixture(scope="module")
def points():
    rnd = random.Random(41)
    pts = [None, o.G1_GEN, o.g1_neg(o.G1_GEN)]
    pts += [o.g1_mul(o.G1_GEN, rnd.randrange(o.R_MOD)) for _ in range(24)]
    assert {sb.is_larger(p[1]) for p in pts if p} == {True, False}
    return pts


def test_field_facts():
    assert P % 4 == 3
    assert sb.SQRT_E == 0xc19139cb84c680a6e14116da060561765e05aa45a1c72a34f082305b61f3f52
    assert sb.SQRT_E.bit_length() == 252 and bin(sb.SQRT_E).count("1") == 109
    # x = 0 and x = 4 have no y: 3 and 67 are non-residues
    assert sb.fq_sqrt(3) is None and sb.fq_sqrt(67) is None
    assert sb.fq_sqrt(4) in (2, P - 2)


def test_uncompressed_equals_oracle_ser_g1(points):
    for p in points:
        assert sb.ser_g1_uncompressed(p) == o.ser_g1(p)


def test_round_trips(points):
    for p in points:
        assert sb.de_g1_uncompressed(sb.ser_g1_uncompressed(p)) == p
        assert sb.de_g1_compressed(sb.ser_g1_compressed(p)) == p
        assert len(sb.ser_g1_compressed(p)) == 32
    for c in (False, True):
        assert sb.de_points(sb.ser_points(points, c), c) == points


def test_compressed_is_x_with_the_flags_of_uncompressed(points):
    for p in points:
        u, c = sb.ser_g1_uncompressed(p), sb.ser_g1_compressed(p)
        assert c[:31] == u[:31] and c[31] & 0x3F == u[31]
        assert c[31] & 0xC0 == u[63] & 0xC0


def _le(v):
    return v.to_bytes(32, "little")


def _reason(fn, b):
    with pytest.raises(sb.BadPoint) as e:
        fn(bytes(b))
    return e.value.reason


def test_rejects_each_malformed_class():
    x, y = o.g1_mul(o.G1_GEN, 77)
    good_u, good_c = sb.ser_g1_uncompressed((x, y)), sb.ser_g1_compressed((x, y))
    # coordinate >= p (x = p, p + 1, 2^254 - 1 after masking)
    for bad in (P, P + 1, (1 << 254) - 1):
        assert _reason(sb.de_g1_compressed, _le(bad)) == sb.NONCANONICAL
        assert _reason(sb.de_g1_uncompressed, _le(bad) + good_u[32:]) == sb.NONCANONICAL
    assert _reason(sb.de_g1_uncompressed, good_u[:32] + _le(P)) == sb.NONCANONICAL
    # all-zero bytes without the infinity flag: x = 0, rhs = 3 is a non-residue
    assert _reason(sb.de_g1_compressed, bytes(32)) == sb.NOT_SQUARE
    assert _reason(sb.de_g1_uncompressed, bytes(64)) == sb.NOT_ON_CURVE
    assert _reason(sb.de_g1_compressed, _le(4)) == sb.NOT_SQUARE
    # infinity flag with a nonzero coordinate, and with the sign flag
    b = bytearray(32)
    b[0], b[31] = 1, sb.INF
    assert _reason(sb.de_g1_compressed, b) == sb.BAD_INFINITY
    assert _reason(sb.de_g1_compressed, bytes(31) + bytes([sb.INF | sb.NEG])) == sb.BAD_INFINITY
    b = bytearray(64)
    b[40], b[63] = 1, sb.INF
    assert _reason(sb.de_g1_uncompressed, b) == sb.BAD_INFINITY
    assert _reason(sb.de_g1_uncompressed, bytes(63) + bytes([sb.INF | sb.NEG])) == sb.BAD_INFINITY
    # a flipped bit in y, a flipped sign flag
    b = bytearray(good_u)
    b[35] ^= 4
    assert _reason(sb.de_g1_uncompressed, b) == sb.NOT_ON_CURVE
    b = bytearray(good_u)
    b[63] ^= sb.NEG
    assert _reason(sb.de_g1_uncompressed, b) == sb.SIGN_FLAG
    # the flipped flag of a compressed point is the other root, not an error
    b = bytearray(good_c)
    b[31] ^= sb.NEG
    assert sb.de_g1_compressed(bytes(b)) == (x, P - y)


def test_de_points_names_the_first_bad_index(points):
    data = bytearray(sb.ser_points(points[1:], True))
    data[32 * 9:32 * 10] = _le(4)
    data[32 * 3:32 * 4] = _le(P)
    with pytest.raises(sb.BadPoint) as e:
        sb.de_points(bytes(data), True)
    assert (e.value.index, e.value.reason) == (3, sb.NONCANONICAL)


def test_rho_is_blake3_low_128_bits():
    import blake3_py
    seed = bytes(range(32))
    for i in (0, 1, 2**32, 2**64 - 1):
        h = blake3_py.blake3(seed + i.to_bytes(8, "little"))
        assert sb.rho(seed, i) == int.from_bytes(h[:16], "little") < 1 << 128
    assert sb.rho(seed, 0) != sb.rho(seed, 1) != sb.rho(bytes(32), 1)


def test_powers_sums_satisfy_tau_relation():
    """tau A == B exactly when the points are powers of one tau"""
    tau, seed = 0x5EED, bytes([7]) * 32
    pts = [o.g1_mul(o.G1_GEN, pow(tau, i, o.R_MOD)) for i in range(5)]
    A, B = sb.powers_sums(pts, seed)
    assert o.g1_mul(A, tau) == B
    pts[3], pts[2] = pts[2], pts[3]
    A, B = sb.powers_sums(pts, seed)
    assert o.g1_mul(A, tau) != B
