"""Operand-edge vectors and the Python-integer reference for the 29-bit-limb
field layer (csrc/field29.h) and the XYZZ arithmetic on it (csrc/curve29.h,
the quad-cooperative forms and the fold in csrc/msm.hip), shared by the host
run (tests/test_field29.py) and the device runs (tests/test_gpu_field29.py,
tests/test_gpu_curve29.py) of qg_selftest_field29 / _curve29 / _msm_fold.

Everything crosses the ABI as raw limbs, so a case can be a non-canonical
representative (x + k p) or carry almost-normalized / lazy limbs, and the
checks read the representation a primitive returned, not only its residue.
A case is asserted only inside the contract the header writes down; the
share of generated cases a contract filter drops is asserted as well.
"""
import ctypes as C
import random

import numpy as np

import quill_oracle as o
from quill_amd._lib import lib

R_MOD, P_MOD = o.R_MOD, o.P_MOD
MODS = {0: R_MOD, 1: P_MOD}
B29 = 1 << 29
RBITS = 261
NORMALIZED, ALMOST, LAZY = B29, B29 + 8, 1 << 31  # exclusive bounds of limbs 0..7

# include/quill_gpu.h
F29 = dict(MUL=0, SQR=1, MULSUB=2, MULT=3, SQRT=4, MULSUBT=5, MULT2=6, SQRT2=7, MULTN3=8, MULTN4=9,
           MULTN3_ALIAS=10, MULTN4_ALIAS=11, NORM=12, NORMFULL=13, RED2P=14, RED6P=15, RED16P=16,
           CANON=17, ISZERO8=18, ISZERO20=19, RELIMB=20)
F29_OP_COUNT = 21
X29 = dict(ADD=0, DBL=1, ADD_AFFINE=2, ACC_FINISH=3, RAW=4, ACC_MADD=5, ADD_Q4=6, DBL_Q4=7)
X29_OP_COUNT = 8
FLAG_MAIN, FLAG_EXC, FLAG_INF = 1, 2, 4
QG_ERR_INVALID, QG_ERR_UNSUPPORTED = -1, -4
MAX_CASES = 65536


# ---- limbs -----------------------------------------------------------------
def limbs(v):
    """normalized limbs of v (the top limb takes everything above 2^232)"""
    assert 0 <= v < 1 << (232 + 32)
    return tuple((v >> (29 * i)) & (B29 - 1) for i in range(8)) + (v >> 232,)


def value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def shaped(low, top_value):
    """limbs 0..7 = low, top limb the largest that keeps the value <= top_value"""
    base = value((low,) * 8 + (0,))
    assert top_value >= base
    return (low,) * 8 + ((top_value - base) >> 232,)


def max_low(l):
    return max(l[:8])


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


# ---- ABI drivers -----------------------------------------------------------
def run_field(ctx, field, op, on_device, cases):
    """cases: tuples of up to 8 limb tuples -> per case 4 result limb tuples"""
    n = len(cases)
    a = np.zeros((max(n, 1), 8, 9), dtype=np.uint32)
    for i, c in enumerate(cases):
        for e, l in enumerate(c):
            a[i, e, :] = l
    out = np.full((max(n, 1), 4, 9), 0xdeadbeef, dtype=np.uint32)
    rc = lib().qg_selftest_field29(ctx, field, op, on_device, _u32p(a), C.c_size_t(n), _u32p(out))
    assert rc == 0, rc
    res = out[:n].tolist()
    return [[tuple(e) for e in r] for r in res]


def run_curve(ctx, op, on_device, cases):
    """cases: (p, q) of 4 limb tuples each (q may be None) -> (points, flags);
    a point is 4 limb tuples; the quad ops give 4 points (lanes 0..3) per case"""
    n = len(cases)
    lanes = 4 if op in (X29["ADD_Q4"], X29["DBL_Q4"]) else 1
    a = np.zeros((max(n, 1), 2, 4, 9), dtype=np.uint32)
    for i, (p, q) in enumerate(cases):
        a[i, 0] = p
        if q is not None:
            a[i, 1] = q
    out = np.full((max(n, 1), lanes, 4, 9), 0xdeadbeef, dtype=np.uint32)
    flags = np.full(max(n, 1), 0xdeadbeef, dtype=np.uint32)
    rc = lib().qg_selftest_curve29(ctx, op, on_device, _u32p(a), C.c_size_t(n), _u32p(out),
                                   _u32p(flags))
    assert rc == 0, rc
    res = out[:n].tolist()
    pts = [[tuple(tuple(c) for c in lane) for lane in r] for r in res]
    if lanes == 1:
        pts = [r[0] for r in pts]
    return pts, [int(f) for f in flags[:n]]


def _words8(v):
    assert 0 <= v < 1 << 256
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


def run_fold(ctx, q4, A, Y, m, batch, istride, want_y):
    """A, Y: batch lists of m points, each 4 plain integers (X, Y, ZZ, ZZZ) ->
    (A_out, Y_out or None) as batch lists of ceil(m / G) such 4-tuples"""
    G = 16 if q4 else 64
    mo = -(-m // G)
    a = np.zeros((batch, istride, 4, 8), dtype=np.uint32)
    y = np.zeros((batch, istride, 4, 8), dtype=np.uint32)
    # the stride's padding is never read: poison it with a non-point
    a[:, m:] = 0xffffffff
    y[:, m:] = 0xffffffff
    for b in range(batch):
        a[b, :m] = [[_words8(c) for c in pt] for pt in A[b]]
        y[b, :m] = [[_words8(c) for c in pt] for pt in Y[b]]
    ao = np.full((batch, mo, 4, 8), 0xdeadbeef, dtype=np.uint32)
    yo = np.full((batch, mo, 4, 8), 0xdeadbeef, dtype=np.uint32)
    rc = lib().qg_selftest_msm_fold(ctx, int(q4), _u32p(a), _u32p(y), m, batch, C.c_size_t(istride),
                                    int(want_y), _u32p(ao), _u32p(yo) if want_y else None)
    assert rc == 0, rc

    def ints(arr):
        return [[tuple(sum(int(w) << (32 * i) for i, w in enumerate(c)) for c in pt) for pt in row]
                for row in arr.tolist()]
    return ints(ao), (ints(yo) if want_y else None)


# ---- field operand classes -------------------------------------------------
class Operand:
    __slots__ = ("l", "v", "name")

    def __init__(self, l, name):
        self.l, self.v, self.name = tuple(l), value(l), name

    def __repr__(self):
        return f"<{self.name} v/p={self.v / P_MOD:.3f} low<={max_low(self.l):#x}>"


_OPERANDS = {}


def operands(p):
    """the issue's operand classes for modulus p: edge values (normalized
    limbs), limb-shape edges (low limbs L, top limb chosen so the value is
    <= T) and seeded random values below 13p"""
    if p in _OPERANDS:
        return _OPERANDS[p]
    ops = []
    for name, v in [("0", 0), ("1", 1), ("p-1", p - 1), ("p", p), ("p+1", p + 1), ("2p-1", 2 * p - 1),
                    ("2p", 2 * p), ("8p-1", 8 * p - 1), ("13p-1", 13 * p - 1),
                    ("2^232-1", (1 << 232) - 1), ("2^232", 1 << 232)]:
        ops.append(Operand(limbs(v), name))
    for lname, low in [("2^29-1", B29 - 1), ("2^29+7", B29 + 7), ("2^31-1", (1 << 31) - 1)]:
        for tname, t in [("2p", 2 * p), ("8p", 8 * p), ("13p", 13 * p)]:
            ops.append(Operand(shaped(low, t), f"L={lname},T={tname}"))
    rnd = random.Random(0x29 + (p & 0xffff))
    for i in range(32):
        ops.append(Operand(limbs(rnd.randrange(13 * p)), f"rand{i}"))
    _OPERANDS[p] = ops
    return ops


def almost(ops):
    return [x for x in ops if max_low(x.l) < ALMOST]


def normalized(ops):
    return [x for x in ops if max_low(x.l) < NORMALIZED]


class Cases:
    """generated cases of one op and the share its contract filter dropped"""

    def __init__(self, generated, keep):
        self.kept = [c for c in generated if keep(c)]
        self.dropped = len(generated) - len(self.kept)
        self.generated = len(generated)

    def assert_share(self):
        # the filter is a condition, not a measurement: at most a third may go
        assert self.generated > 0 and 3 * self.dropped <= self.generated, (self.dropped, self.generated)


def mul_cases(p):
    """one operand almost-normalized, the other at most lazy; a b <= 2^261 p"""
    ops = operands(p)
    return Cases([(a, b) for a in almost(ops) for b in ops], lambda c: c[0].v * c[1].v <= (p << RBITS))


def sqr_cases(p):
    return Cases([(a,) for a in almost(operands(p))], lambda c: c[0].v ** 2 <= (p << RBITS))


def mulsub_cases(p):
    """a, b, c, d almost-normalized, c d < 4p 2^261, c's limbs < 2^30: every
    (c, d) pair with a rotating (a, b) pair, and every (a, b) with a rotating
    (c, d)"""
    al = almost(operands(p))
    pairs = [(x, y) for x in al for y in al]
    gen = []
    for i, (c, d) in enumerate(pairs):
        a, b = pairs[(7 * i + 3) % len(pairs)]
        gen.append((a, b, c, d))
    for i, (a, b) in enumerate(pairs):
        c, d = pairs[(11 * i + 5) % len(pairs)]
        gen.append((a, b, c, d))
    return Cases(gen, lambda c: c[2].v * c[3].v < ((4 * p) << RBITS) and max(c[2].l) < (1 << 30))


def check_mul(p, a, b, r, what):
    v = value(r)
    assert v % p == a.v * b.v * pow(2, -RBITS, p) % p, (what, a, b)
    assert v < 2 * p and max_low(r) < NORMALIZED, (what, a, b, v / p)


def check_mulsub(p, a, b, c, d, r, what):
    v = value(r)
    assert v % p == (a.v * b.v - c.v * d.v) * pow(2, -RBITS, p) % p, (what, a, b, c, d)
    # value < a b 2^-261 + 5p, normalized
    assert (v << RBITS) < a.v * b.v + ((5 * p) << RBITS) and max_low(r) < NORMALIZED, (what, a, b, c, d)


def unary_cases(p):
    """op -> operands inside the op's written contract"""
    ops = operands(p)
    wide = [Operand((0xffffffff,) * 8 + (5,), "limbs 2^32-1"),
            Operand((0xffffffff, 0) * 4 + (0,), "alternating 2^32-1")]
    zero20 = [Operand(limbs(k * p + d), f"{k}p{d:+d}") for k in range(20) for d in (-1, 0, 1)
              if k * p + d >= 0]
    # a multiple's low limb under other upper limbs: passes the one-multiply
    # filter and has to fail the exact comparison
    zero20 += [Operand(limbs(k * p + (j << 29)), f"{k}p+{j}*2^29") for k in range(20) for j in (1, 1 << 100)]
    zero20 += normalized(ops)

    def below(bound):
        """values under a reduction's bound: the classes that fit, every class
        folded under the bound, the bound's edge, and limb-wise sums of two
        normalized values (the lazy shape add29 makes)"""
        xs = [x for x in ops if x.v < bound]
        nz = [Operand(limbs(x.v % bound), f"{x.name} mod bound") for x in ops]
        nz.append(Operand(limbs(bound - 1), "bound-1"))
        xs += nz
        for x, y in zip(nz, nz[1:]):
            if x.v + y.v < bound:
                xs.append(Operand(tuple(a + b for a, b in zip(x.l, y.l)), f"{x.name}+{y.name}"))
        return xs

    return {
        "NORM": ops + wide,
        "NORMFULL": ops,  # lazy at most: its carry is added in 32 bits
        "RED2P": below(4 * p),
        "RED6P": below(6 * p),
        "RED16P": below(16 * p),
        "CANON": [x for x in normalized(ops) if x.v < 2 * p] + [Operand(limbs(x.v % (2 * p)), "r") for x in ops],
        "ISZERO8": [x for x in zero20 if x.v < 8 * p],
        "ISZERO20": [x for x in zero20 if x.v < 20 * p],
        "RELIMB": [x for x in normalized(ops) if x.v < 1 << 256] + [Operand(limbs((1 << 256) - 1), "2^256-1")],
    }


def check_unary(p, name, a, r):
    v = value(r)
    if name == "NORM":
        assert v == a.v and max_low(r) < ALMOST, (name, a)
    elif name == "NORMFULL":
        assert v == a.v and max_low(r) < NORMALIZED, (name, a)
    elif name in ("RED2P", "RED6P", "RED16P"):
        assert v % p == a.v % p and v < 2 * p and max_low(r) < NORMALIZED, (name, a, v / p)
    elif name == "CANON":
        assert v == a.v % p and max_low(r) < NORMALIZED, (name, a)
    elif name in ("ISZERO8", "ISZERO20"):
        assert r == (int(a.v % p == 0),) + (0,) * 8, (name, a)
    elif name == "RELIMB":
        assert r == a.l, (name, a)
    else:
        raise AssertionError(name)


def check_field_hd(ctx, field, on_device):
    """the host-callable primitives of one field, host or device build; returns
    {op: [result limbs]} of the product ops so a caller can compare builds"""
    p = MODS[field]
    got = {}
    mc = mul_cases(p)
    mc.assert_share()
    res = run_field(ctx, field, F29["MUL"], on_device, [(a.l, b.l) for a, b in mc.kept])
    for (a, b), r in zip(mc.kept, res):
        check_mul(p, a, b, r[0], "mul29")
        assert r[1:] == [(0,) * 9] * 3
    got["MUL"] = [r[0] for r in res]
    sc = sqr_cases(p)
    sc.assert_share()
    res = run_field(ctx, field, F29["SQR"], on_device, [(a.l,) for a, in sc.kept])
    for (a,), r in zip(sc.kept, res):
        check_mul(p, a, a, r[0], "sqr29")
    got["SQR"] = [r[0] for r in res]
    ms = mulsub_cases(p)
    ms.assert_share()
    res = run_field(ctx, field, F29["MULSUB"], on_device, [tuple(x.l for x in c) for c in ms.kept])
    for c, r in zip(ms.kept, res):
        check_mulsub(p, *c, r[0], "mulsub29")
    got["MULSUB"] = [r[0] for r in res]
    for name, xs in unary_cases(p).items():
        assert len(xs) >= 20, name
        res = run_field(ctx, field, F29[name], on_device, [(a.l,) for a in xs])
        for a, r in zip(xs, res):
            check_unary(p, name, a, r[0])
    return got


def check_field_device_only(ctx, field, hd):
    """mul29t, sqr29t, mulsub29t, mul29t2, sqr29t2, mul29tn<3>, <4> on the
    device: each inside the contract, limb for limb equal to the plain form
    (`hd`: check_field_hd's device results), the interleaved forms equal to
    separate calls"""
    p = MODS[field]
    mc, sc, ms = mul_cases(p).kept, sqr_cases(p).kept, mulsub_cases(p).kept
    mt = [r[0] for r in run_field(ctx, field, F29["MULT"], 1, [(a.l, b.l) for a, b in mc])]
    for (a, b), r in zip(mc, mt):
        check_mul(p, a, b, r, "mul29t")
    assert mt == hd["MUL"]
    st = [r[0] for r in run_field(ctx, field, F29["SQRT"], 1, [(a.l,) for a, in sc])]
    for (a,), r in zip(sc, st):
        check_mul(p, a, a, r, "sqr29t")
    assert st == hd["SQR"]
    mst = [r[0] for r in run_field(ctx, field, F29["MULSUBT"], 1, [tuple(x.l for x in c) for c in ms])]
    for c, r in zip(ms, mst):
        check_mulsub(p, *c, r, "mulsub29t")
    assert mst == hd["MULSUB"]
    # interleaved chains: product i beside products at co-prime strides, so
    # every operand class meets every position of the interleave
    n = len(mc)
    idx = [[(i + k * 97) % n for k in range(4)] for i in range(n)]
    res = run_field(ctx, field, F29["MULT2"], 1,
                    [(mc[j[0]][0].l, mc[j[0]][1].l, mc[j[1]][0].l, mc[j[1]][1].l) for j in idx])
    for j, r in zip(idx, res):
        assert r[0] == mt[j[0]] and r[1] == mt[j[1]], ("mul29t2", mc[j[0]], mc[j[1]])
    ns = len(sc)
    res = run_field(ctx, field, F29["SQRT2"], 1, [(sc[i][0].l, sc[(i + 5) % ns][0].l) for i in range(ns)])
    for i, r in enumerate(res):
        assert r[0] == st[i] and r[1] == st[(i + 5) % ns], ("sqr29t2", sc[i])
    for N, plain, alias in ((3, "MULTN3", "MULTN3_ALIAS"), (4, "MULTN4", "MULTN4_ALIAS")):
        cases = []
        for j in idx:
            c = [(0,) * 9] * 8
            for k in range(N):
                c[k], c[4 + k] = mc[j[k]][0].l, mc[j[k]][1].l
            cases.append(tuple(c))
        for op in (plain, alias):
            res = run_field(ctx, field, F29[op], 1, cases)
            for j, r in zip(idx, res):
                assert r[:N] == [mt[j[k]] for k in range(N)], (op, j)
                assert r[N:] == [(0,) * 9] * (4 - N)


# ---- G1 in the R = 2^261 domain ---------------------------------------------
P = P_MOD
RM = pow(2, RBITS, P)
RINV = pow(2, -RBITS, P)
ONE = limbs(RM)
ZERO = (0,) * 9
INF = (ZERO, ONE, ZERO, ZERO)


def small_multiples(n):
    """[None, G, 2G, ..., nG] affine: one Jacobian accumulation and one batch
    inversion"""
    jac = []
    acc = (0, 1, 0)
    g = (o.G1_GEN[0], o.G1_GEN[1], 1)
    for _ in range(n):
        acc = o._jac_add(acc, g)
        jac.append(acc)
    pre = [1]
    for _, _, z in jac:
        pre.append(pre[-1] * z % P)
    inv = pow(pre[-1], -1, P)
    out = [None] * (n + 1)
    for i in range(n - 1, -1, -1):
        x, y, z = jac[i]
        zi = inv * pre[i] % P
        inv = inv * z % P
        out[i + 1] = (x * zi * zi % P, y * zi * zi * zi % P)
    return out


NMULT = 1024
_MULT = []


def kG(k):
    """affine k G for |k| <= NMULT (None for 0)"""
    if not _MULT:
        _MULT.extend(small_multiples(NMULT))
    return _MULT[k] if k >= 0 else o.g1_neg(_MULT[-k])


_MUL_CACHE = {}


def sG(s):
    """affine s G for any integer s"""
    s %= R_MOD
    if s not in _MUL_CACHE:
        _MUL_CACHE[s] = o.g1_mul(o.G1_GEN, s)
    return _MUL_CACHE[s]


def mulG(k):
    """affine k G: from the table where it reaches, else by the oracle"""
    return kG(k) if abs(k) <= NMULT else sG(k)


def xyzz_ints(pt, rnd, lift=0):
    """a random XYZZ representative of affine pt as integers in the R = 2^261
    domain, each coordinate + p where its bit of `lift` is set (X, Y, ZZ, ZZZ)"""
    if pt is None:
        return (0, RM, 0, 0)
    z = rnd.randrange(2, P)
    zz, zzz = z * z % P, z * z * z % P
    c = [pt[0] * zz * RM % P, pt[1] * zzz * RM % P, zz * RM % P, zzz * RM % P]
    return tuple(v + (P if (lift >> i) & 1 else 0) for i, v in enumerate(c))


def xyzz(pt, rnd, lift=0):
    return tuple(limbs(v) for v in xyzz_ints(pt, rnd, lift))


def affine_mont(pt):
    """canonical affine coordinates in the R = 2^261 domain (an MSM table row)"""
    return (limbs(pt[0] * RM % P), limbs(pt[1] * RM % P), ZERO, ZERO)


def is_inf(pt4):
    return all(x == 0 for x in pt4[2])


def assert_point(pt4, want, bounds, what):
    """pt4 (4 limb tuples) represents affine `want`: X = x ZZ, Y = y ZZZ,
    ZZ^3 = ZZZ^2 != 0 (no inversion); bounds: per coordinate (value bound in
    units of p, exclusive bound of limbs 0..7)"""
    if want is None:
        assert is_inf(pt4), (what, "expected infinity")
        return
    X, Y, ZZ, ZZZ = (value(c) for c in pt4)
    for c, (vb, lb), nm in zip(pt4, bounds, ("X", "Y", "ZZ", "ZZZ")):
        assert value(c) < vb * P and max_low(c) < lb, (what, nm, value(c) / P, hex(max_low(c)))
    zz, zzz = ZZ * RINV % P, ZZZ * RINV % P
    assert zz != 0 and pow(zz, 3, P) == zzz * zzz % P, (what, "ZZ^3 != ZZZ^2")
    assert X * RINV % P == want[0] * zz % P, (what, "x")
    assert Y * RINV % P == want[1] * zzz % P, (what, "y")


OUT2P = ((2, NORMALIZED),) * 4                                           # curve29.h:5
ACC_INV = ((16, ALMOST), (8, NORMALIZED), (2, NORMALIZED), (2, NORMALIZED))  # curve29.h:82


# ---- x29_add / x29_dbl / the quad forms -------------------------------------
NINV = -pow(P, -1, 1 << RBITS) % (1 << RBITS)


def mont(a, b):
    """the integer mul29 returns: (a b + m p) 2^-261, m = -a b / p mod 2^261"""
    t = a * b
    return (t + t * NINV % (1 << RBITS) * P) >> RBITS


def split_pair(pa, pb, rnd, which):
    """representatives p of pa and q of pb (pb = +-pa) whose cross products
    U1 = X1 ZZ2 / U2 = X2 ZZ1 (which = 0) or S1 / S2 (which = 1) come out of
    mul29 as different integers of one residue: P (or R) is then a nonzero
    multiple of p whose limbs only a full carry propagation normalizes.  A
    Montgomery product of operands < 2p exceeds p about once in 40."""
    for _ in range(4000):
        p, q = xyzz_ints(pa, rnd, 15), xyzz_ints(pb, rnd, 15)
        if mont(p[which], q[2 + which]) != mont(q[which], p[2 + which]):
            return tuple(limbs(v) for v in p), tuple(limbs(v) for v in q)
    raise AssertionError("no split representatives found")


def add_cases(seed):
    """(p, q, expected affine sum, kind); neighbouring cases take different
    branches: regular, doubling, cancellation, infinity operands"""
    rnd = random.Random(seed)
    cases = []
    for i in range(96):
        a, b = rnd.randrange(1, NMULT // 2), rnd.randrange(1, NMULT // 2)
        if a == b:
            b += 1
        lp, lq = rnd.randrange(16), rnd.randrange(16)
        if i % 16 == 15:
            lp, lq = 15, 15
        kind = ("reg", "dbl", "reg", "neg", "reg", "inf+q", "p+inf", "inf+inf")[i % 8]
        if kind == "reg":
            cases.append((xyzz(kG(a), rnd, lp), xyzz(kG(b), rnd, lq), kG(a + b), kind))
        elif kind == "dbl":  # the same point under another z
            if (i // 8) % 3 < 2:  # ... with P (then R) = k p, k != 4
                p, q = split_pair(kG(a), kG(a), rnd, (i // 8) % 3)
            else:
                p, q = xyzz(kG(a), rnd, lp), xyzz(kG(a), rnd, lq)
            cases.append((p, q, kG(2 * a), kind))
        elif kind == "neg":
            if (i // 8) % 2 == 0:
                p, q = split_pair(kG(a), kG(-a), rnd, 0)
            else:
                p, q = xyzz(kG(a), rnd, lp), xyzz(kG(-a), rnd, lq)
            cases.append((p, q, None, kind))
        elif kind == "inf+q":
            cases.append((INF, xyzz(kG(b), rnd, lq), kG(b), kind))
        elif kind == "p+inf":
            cases.append((xyzz(kG(a), rnd, lp), INF, kG(a), kind))
        else:
            cases.append((INF, INF, None, kind))
    return cases


def dbl_cases(seed):
    rnd = random.Random(seed)
    cases = []
    for i in range(48):
        a = rnd.randrange(1, NMULT // 2)
        if i % 4 == 3:
            cases.append((INF, None, "inf"))
        else:
            cases.append((xyzz(kG(a), rnd, 15 if i % 8 == 0 else rnd.randrange(16)), kG(2 * a), "reg"))
    return cases


def check_curve_hd(ctx, on_device):
    """x29_add, x29_dbl, x29_add_affine, x29_acc_finish, x29_raw/unraw: host
    or device build; returns the add / dbl results for the quad comparison"""
    ac = add_cases(11)
    add, fl = run_curve(ctx, X29["ADD"], on_device, [(p, q) for p, q, _, _ in ac])
    assert fl == [0] * len(ac)
    for (p, q, want, kind), r in zip(ac, add):
        assert_point(r, want, OUT2P, ("x29_add", kind))
        if kind == "inf+q":
            assert r == q
        if kind == "p+inf":
            assert r == p
    dc = dbl_cases(12)
    dbl, _ = run_curve(ctx, X29["DBL"], on_device, [(p, None) for p, _, _ in dc])
    for (p, want, kind), r in zip(dc, dbl):
        assert_point(r, want, OUT2P, ("x29_dbl", kind))
    # madd-2008-s on a < 2p accumulator: p + affine a, a == p, a == -p, p inf
    rnd = random.Random(13)
    mc = []
    for i in range(64):
        a, b = rnd.randrange(1, NMULT // 2), rnd.randrange(1, NMULT // 2)
        if a == b:
            b += 1
        kind = ("reg", "dbl", "reg", "neg", "reg", "inf")[i % 6]
        lp = rnd.randrange(16)
        if kind == "reg":
            mc.append((xyzz(kG(a), rnd, lp), affine_mont(kG(b)), kG(a + b)))
        elif kind == "dbl":
            mc.append((xyzz(kG(a), rnd, lp), affine_mont(kG(a)), kG(2 * a)))
        elif kind == "neg":
            mc.append((xyzz(kG(a), rnd, lp), affine_mont(kG(-a)), None))
        else:
            mc.append((INF, affine_mont(kG(b)), kG(b)))
    res, _ = run_curve(ctx, X29["ADD_AFFINE"], on_device, [(p, q) for p, q, _ in mc])
    for (p, q, want), r in zip(mc, res):
        assert_point(r, want, OUT2P, "x29_add_affine")
    # x29_acc_finish: a lazily reduced accumulator at the top of its bounds
    fc = []
    for i in range(64):
        a = rnd.randrange(1, NMULT)
        c = list(xyzz_ints(kG(a), rnd, (rnd.randrange(4)) << 2))
        c[0] += (15, 14, 0, rnd.randrange(16))[i % 4] * P
        c[1] += (7, 6, 0, rnd.randrange(8))[i % 4] * P
        fc.append((tuple(limbs(v) for v in c), kG(a)))
    fc.append((INF, None))
    res, _ = run_curve(ctx, X29["ACC_FINISH"], on_device, [(p, None) for p, _ in fc])
    for (p, want), r in zip(fc, res):
        assert_point(r, want, OUT2P, "x29_acc_finish")
        assert r[2:] == p[2:]
    # x29_raw / x29_unraw: any 36 words come back unchanged
    rc = [(tuple(tuple(rnd.randrange(1 << 32) for _ in range(9)) for _ in range(4)), None) for _ in range(32)]
    res, _ = run_curve(ctx, X29["RAW"], on_device, rc)
    assert res == [p for p, _ in rc]
    return ac, add, dc, dbl


# ---- x29_acc_madd_tp --------------------------------------------------------
class Acc:
    """an accumulator case: limbs handed to the device and the affine value"""

    def __init__(self, pt4, k):
        self.pt4, self.k = pt4, k


def madd_start(i, rnd):
    """accumulator a G at a worst-case representative (the issue's grid)"""
    a = rnd.randrange(1, 256)
    c = list(xyzz_ints(kG(a), rnd, (i & 3) << 2))  # ZZ, ZZZ optionally + p
    c[0] += (0, 14, 15, rnd.randrange(16))[(i >> 2) & 3] * P
    c[1] += (0, 7, rnd.randrange(8))[i % 3] * P
    assert c[0] < 16 * P and c[1] < 8 * P
    return Acc(tuple(limbs(v) for v in c), a)


def madd_step(ctx, accs, step, rnd):
    """one x29_acc_madd_tp (+ exc) per live accumulator with a fresh point:
    every 7th case the accumulator's negative, every 11th the accumulator
    itself.  Asserts flag, invariant (curve29.h:82) and affine sum; returns
    the accumulators to carry on with (cancelled ones leave the chain)."""
    cases, bs = [], []
    for i, acc in enumerate(accs):
        j = i + step
        if j % 7 == 0:
            b = -acc.k
        elif j % 11 == 0:
            b = acc.k
        else:
            b = rnd.randrange(1, 8)
            if b == acc.k:
                b += 1
        bs.append(b)
        cases.append((acc.pt4, affine_mont(mulG(b))))
    res, flags = run_curve(ctx, X29["ACC_MADD"], 1, cases)
    nxt = []
    stats = [0.0, 0.0]
    for acc, b, r, f in zip(accs, bs, res, flags):
        what = ("x29_acc_madd_tp", step, acc.k, b)
        if b == -acc.k:
            assert f == FLAG_EXC | FLAG_INF, what
            assert r == acc.pt4, what  # untouched: the caller drops it
            continue
        assert f == (FLAG_EXC if b == acc.k else FLAG_MAIN), what
        assert_point(r, mulG(acc.k + b), ACC_INV, what)
        stats = [max(stats[0], value(r[0]) / P), max(stats[1], value(r[1]) / P)]
        nxt.append(Acc(r, acc.k + b))
    return nxt, stats


# ---- the fold ---------------------------------------------------------------
FOLD_M = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)
FOLD_PATTERNS = ("distinct", "equal_A", "alternating_Y", "scattered_inf", "all_inf")


def fold_scalars(pattern, m, rnd):
    """(a_e, y_e) as multiples of G (0 = infinity)"""
    if pattern == "distinct":
        return [rnd.randrange(1, NMULT) for _ in range(m)], [rnd.randrange(1, NMULT) for _ in range(m)]
    if pattern == "equal_A":  # every tree step of A doubles; so does every scan step of Y
        a, y = rnd.randrange(1, NMULT), rnd.randrange(1, NMULT)
        return [a] * m, [y] * m
    if pattern == "alternating_Y":  # suffix sums cancel to infinity
        q = rnd.randrange(1, NMULT)
        return [rnd.randrange(1, NMULT) for _ in range(m)], [q if e % 2 == 0 else -q for e in range(m)]
    if pattern == "scattered_inf":
        return ([0 if rnd.randrange(3) == 0 else rnd.randrange(1, NMULT) for _ in range(m)],
                [0 if rnd.randrange(3) == 0 else rnd.randrange(1, NMULT) for _ in range(m)])
    assert pattern == "all_inf"
    return [0] * m, [0] * m


def assert_fold_point(c4, want, last, what):
    """a fold output (4 plain integers): the R = 2^261 word layout < 2p, or,
    from the last level, canonical in the host's 2^256 Montgomery form"""
    X, Y, ZZ, ZZZ = c4
    if want is None:
        assert ZZ == 0, (what, "expected infinity")
        if last:
            assert c4 == (0, (1 << 256) % P, 0, 0), what
        return
    bound, rinv = (P, pow(2, -256, P)) if last else (2 * P, RINV)
    assert all(v < bound for v in c4), (what, [v / P for v in c4])
    zz, zzz = ZZ * rinv % P, ZZZ * rinv % P
    assert zz != 0 and pow(zz, 3, P) == zzz * zzz % P, (what, "ZZ^3 != ZZZ^2")
    assert X * rinv % P == want[0] * zz % P, (what, "x")
    assert Y * rinv % P == want[1] * zzz % P, (what, "y")


def fold_affine(c4):
    """affine value of a fold output in the R = 2^261 layout"""
    X, Y, ZZ, ZZZ = c4
    if ZZ == 0:
        return None
    return (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)


def check_fold(ctx, q4, want_y, batch, m, pattern, seed):
    rnd = random.Random(seed)
    G = 16 if q4 else 64
    mo = -(-m // G)
    istride = m + 1 + seed % 5
    sc = [fold_scalars(pattern, m, rnd) for _ in range(batch)]
    A = [[xyzz_ints(kG(k), rnd, rnd.randrange(16)) for k in a] for a, _ in sc]
    Y = [[xyzz_ints(kG(k), rnd, rnd.randrange(16)) for k in y] for _, y in sc]
    Ao, Yo = run_fold(ctx, q4, A, Y, m, batch, istride, want_y)
    for b in range(batch):
        a, y = sc[b]
        what = (pattern, "q4" if q4 else "q1", "want_y" if want_y else "last", m, b)
        for w in range(mo):
            grp = range(w * G, min(m, (w + 1) * G))
            sa = sum(a[e] + (e - w * G) * y[e] for e in grp)
            sy = G * sum(y[e] for e in grp)
            assert_fold_point(Ao[b][w], sG(sa), not want_y, what + (w, "A"))
            if want_y:
                assert_fold_point(Yo[b][w], sG(sy), False, what + (w, "Y"))
        if want_y:
            # the level invariant, summed from what the kernel wrote
            tot = None
            for w in range(mo):
                tot = o.g1_add(tot, o.g1_add(fold_affine(Ao[b][w]), o.g1_mul(fold_affine(Yo[b][w]), w)))
            assert tot == sG(sum(a[e] + e * y[e] for e in range(m))), what
