"""ark-serialize encodings of a G1Affine point and the multipliers of the SRS
powers check, restated in Python for the tests of the device import / export
(qg_srs_import, qg_srs_export, qg_srs_check_powers).

Flags sit in the top two bits of a point's LAST byte: bit 7 = y is the larger
root (y > p - y), bit 6 = the point at infinity.  Uncompressed is x || y (64
bytes, the rules of `_Reader.g1` in quill_amd/serialize.py); compressed is x
alone (32 bytes) with the same flags, y recovered as a square root of x^3 + 3
(p = 3 mod 4, so rhs^((p+1)/4)).  No ark-serialize source is at hand: the
compressed form is pinned by this convention only.

A malformed encoding raises BadPoint(reason) with the reason codes of
include/quill_gpu.h (QG_SRS_BAD_*)."""
import blake3_py
import quill_oracle as o

P = o.P_MOD
INF, NEG = 0x40, 0x80
NONCANONICAL, BAD_INFINITY, NOT_SQUARE, NOT_ON_CURVE, SIGN_FLAG = 1, 2, 3, 4, 5
SQRT_E = (P + 1) // 4


class BadPoint(ValueError):
    def __init__(self, reason):
        self.reason = reason
        super().__init__(f"malformed point (reason {reason})")


def is_larger(y: int) -> bool:
    return y > P - y


def fq_sqrt(a: int):
    """a square root of a mod p, or None"""
    y = pow(a, SQRT_E, P)
    return y if y * y % P == a % P else None


def ser_g1_uncompressed(pt) -> bytes:
    if pt is None:
        return bytes(63) + bytes([INF])
    x, y = pt
    b = bytearray(x.to_bytes(32, "little") + y.to_bytes(32, "little"))
    if is_larger(y):
        b[63] |= NEG
    return bytes(b)


def ser_g1_compressed(pt) -> bytes:
    if pt is None:
        return bytes(31) + bytes([INF])
    x, y = pt
    b = bytearray(x.to_bytes(32, "little"))
    if is_larger(y):
        b[31] |= NEG
    return bytes(b)


def _split_flags(b: bytes):
    b = bytearray(b)
    flags = b[-1] & 0xC0
    b[-1] &= 0x3F
    return b, flags


def de_g1_uncompressed(b: bytes):
    assert len(b) == 64
    b, flags = _split_flags(b)
    x, y = int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little")
    if flags & INF:
        if x or y or flags & NEG:
            raise BadPoint(BAD_INFINITY)
        return None
    if x >= P or y >= P:
        raise BadPoint(NONCANONICAL)
    if (y * y - x * x * x - 3) % P:
        raise BadPoint(NOT_ON_CURVE)
    if bool(flags & NEG) != is_larger(y):
        raise BadPoint(SIGN_FLAG)
    return (x, y)


def de_g1_compressed(b: bytes):
    assert len(b) == 32
    b, flags = _split_flags(b)
    x = int.from_bytes(b, "little")
    if flags & INF:
        if x or flags & NEG:
            raise BadPoint(BAD_INFINITY)
        return None
    if x >= P:
        raise BadPoint(NONCANONICAL)
    y = fq_sqrt((x * x * x + 3) % P)
    if y is None:
        raise BadPoint(NOT_SQUARE)
    if is_larger(y) != bool(flags & NEG):
        y = P - y
    return (x, y)


def ser_points(points, compressed: bool) -> bytes:
    enc = ser_g1_compressed if compressed else ser_g1_uncompressed
    return b"".join(enc(p) for p in points)


def de_points(data: bytes, compressed: bool):
    """the points, or raises BadPoint with .index = the first bad point"""
    pb, dec = (32, de_g1_compressed) if compressed else (64, de_g1_uncompressed)
    assert len(data) % pb == 0
    out = []
    for i in range(len(data) // pb):
        try:
            out.append(dec(data[i * pb:(i + 1) * pb]))
        except BadPoint as e:
            e.index = i
            raise
    return out


def rho(seed: bytes, i: int) -> int:
    """multiplier i of the powers check: the low 128 bits, little-endian, of
    BLAKE3(seed || u64_le(i))"""
    assert len(seed) == 32
    return int.from_bytes(blake3_py.blake3(seed + i.to_bytes(8, "little"))[:16], "little")


def powers_sums(points, seed: bytes):
    """(A, B) of the powers check over ALL N points: A = sum_{i<N-1} rho_i P_i,
    B = sum_{1<=j<N} rho_{j-1} P_j (oracle scalar multiplications)"""
    N = len(points)
    A = B = None
    for i in range(N - 1):
        r = rho(seed, i)
        A = o.g1_add(A, o.g1_mul(points[i], r))
        B = o.g1_add(B, o.g1_mul(points[i + 1], r))
    return A, B
