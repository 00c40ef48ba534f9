"""CPU check of the 29-bit-limb Montgomery layer (csrc/field29.h, host build):
mul29 = a*b*2^-261 mod p with output < 2p, lazy add/sub + normalisation, the
2p / p conditional subtractions.  Python integers are the reference."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
RINV = pow(2, -261, P)


@pytest.fixture(scope="module")
def raw():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    d = tempfile.mkdtemp()
    exe = os.path.join(d, "f29")
    subprocess.run([gxx, "-O2", "-std=c++17", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "field29_check.cpp")], check=True)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode()
    shutil.rmtree(d, ignore_errors=True)
    res = []
    for line in out.strip().splitlines():
        res.append({k: int(v, 16) for k, v in (kv.split("=") for kv in line.split())})
    return res


@pytest.fixture(scope="module")
def rows(raw):
    return [r for r in raw if "a" in r]


def test_mul29(rows):
    for r in rows:
        assert r["m"] % P == r["a"] * r["b"] * RINV % P
        assert r["m"] < 2 * P


def test_sub_then_mul(rows):
    for r in rows:
        assert r["md"] % P == (r["a"] - r["b"]) * r["c"] * RINV % P
        assert r["md"] < 2 * P


def test_reduce_and_canon(rows):
    for r in rows:
        assert r["r"] < 2 * P and r["r"] % P == (r["m"] + r["c"]) % P
        assert r["cm"] == r["m"] % P


def test_lazy_operand(rows):
    for r in rows:
        assert r["lz"] % P == (r["a"] + r["b"]) * r["c"] * RINV % P


def test_square(rows):
    for r in rows:
        assert r["sq"] % P == (r["a"] - r["b"]) ** 2 * RINV % P
        assert r["sq"] < 2 * P


def test_mulsub(rows):
    for r in rows:
        assert r["ms"] % P == (r["a"] * (r["b"] - r["c"]) - r["c"] * r["m"]) * RINV % P
        assert r["ms"] < 6 * P


def test_fast_zero_mod_p(raw):
    """is_zero_mod29_fast (the one-multiply residue filter used by the MSM's
    curve additions) agrees with the exhaustive multiple-of-p comparison."""
    z = [r for r in raw if "zerotest" in r]
    assert z and z[0]["zerotest"] == 1


# ---- the same primitives through qg_selftest_field29 / _curve29 ------------
# (host build of the library; operand-edge vectors of tests/field29_vectors.py,
# which the GPU tests run again on the gfx950 build)
@pytest.mark.parametrize("field", [0, 1], ids=["Fr", "Fq"])
def test_field29_edges_host(field):
    import field29_vectors as fv
    fv.check_field_hd(None, field, 0)


def test_field29_filter_share():
    """the contract filters drop at most a third of the generated pairs"""
    import field29_vectors as fv
    for p in fv.MODS.values():
        for cases in (fv.mul_cases(p), fv.sqr_cases(p), fv.mulsub_cases(p)):
            cases.assert_share()
            assert len(cases.kept) >= 40


def test_field29_device_only_forms_have_no_host_path():
    import field29_vectors as fv
    for op in ("MULT", "SQRT", "MULSUBT", "MULT2", "SQRT2", "MULTN3", "MULTN4", "MULTN3_ALIAS",
               "MULTN4_ALIAS"):
        a = (C.c_uint32 * 72)()
        out = (C.c_uint32 * 36)()
        for field in (0, 1):
            assert fv.lib().qg_selftest_field29(None, field, fv.F29[op], 0, a, 1, out) == fv.QG_ERR_UNSUPPORTED
    fl = (C.c_uint32 * 1)()
    for op in ("ACC_MADD", "ADD_Q4", "DBL_Q4"):
        a = (C.c_uint32 * 72)()
        out = (C.c_uint32 * 144)()
        assert fv.lib().qg_selftest_curve29(None, fv.X29[op], 0, a, 1, out, fl) == fv.QG_ERR_UNSUPPORTED


def test_curve29_host():
    """x29_add / x29_dbl / x29_add_affine / x29_acc_finish / x29_raw on the
    host build: regular, doubling, cancellation and infinity operands, with
    coordinates canonical and + p"""
    import field29_vectors as fv
    fv.check_curve_hd(None, 0)


def test_redundant_subtrahend_constants():
    """l9_redundant(k p) (K2, K4, K9, K17: limb i of k p plus 2^29 - 1, limb 0
    plus 2^29, the top limb minus 1) leaves no negative limb in k - b for an
    almost-normalized b only while limbs 1..7 of k p are at least 8 and its
    top limb at least 1 (limb 0 of b is below 2^29: norm29 masks it and adds
    no carry).  A property of the two moduli, checked here because sub29 /
    subk29 rely on it without a test of their own."""
    import field29_vectors as fv
    for p in fv.MODS.values():
        for k in (2, 4, 9, 17):
            l = fv.limbs(k * p)
            red = (l[0] + fv.B29,) + tuple(x + fv.B29 - 1 for x in l[1:8]) + (l[8] - 1,)
            assert fv.value(red) == k * p
            assert red[0] >= fv.NORMALIZED - 1 and min(red[1:8]) >= fv.ALMOST - 1 and red[8] >= 0, k
