"""The XYZZ device primitives on the 29-bit-limb field (csrc/curve29.h and
the quad-cooperative forms and fold of csrc/msm.hip) through
qg_selftest_curve29 / qg_selftest_msm_fold, against Python integers and the
oracle's G1 (tests/field29_vectors.py): the bucket accumulator's madd at the
top of its written invariant and as an inductive chain, x29_add / x29_dbl
and their quad forms on regular, doubling, cancelling and infinity operands
packed side by side in one wave, and k_msm_wfold on partial groups and
degenerate element patterns."""
import random

import pytest

import field29_vectors as fv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def single(dev):
    """(add cases, x29_add results, dbl cases, x29_dbl results) on the device,
    each asserted against the reference"""
    return fv.check_curve_hd(dev.h, 1)


def test_single_lane_ops_match_host_build(single):
    ac, add, dc, dbl = single
    _, hadd, _, hdbl = fv.check_curve_hd(None, 0)
    assert add == hadd and dbl == hdbl


def test_add_q4(dev, single):
    """every lane of the quad returns x29_add's limbs; neighbouring quads take
    the regular path, the P == 0 fallback (doubling, cancellation) and the
    infinity returns"""
    ac, add, _, _ = single
    kinds = [k for _, _, _, k in ac]
    assert {"reg", "dbl", "neg", "inf+q", "p+inf", "inf+inf"} <= set(kinds[:16])  # within one wave
    res, _ = fv.run_curve(dev.h, fv.X29["ADD_Q4"], 1, [(p, q) for p, q, _, _ in ac])
    for (p, q, want, kind), lanes, one in zip(ac, res, add):
        for lane in lanes:
            fv.assert_point(lane, want, fv.OUT2P, ("x29_add_q4", kind))
        assert lanes == [one] * 4, kind


def test_dbl_q4(dev, single):
    _, _, dc, dbl = single
    res, _ = fv.run_curve(dev.h, fv.X29["DBL_Q4"], 1, [(p, None) for p, _, _ in dc])
    for (p, want, kind), lanes, one in zip(dc, res, dbl):
        for lane in lanes:
            fv.assert_point(lane, want, fv.OUT2P, ("x29_dbl_q4", kind))
        assert lanes == [one] * 4, kind


def test_q4_partial_wave(dev, single):
    """a launch whose last wave is partly empty (whole quads leave)"""
    ac, add, _, _ = single
    for n in (1, 3, 17):
        res, _ = fv.run_curve(dev.h, fv.X29["ADD_Q4"], 1, [(p, q) for p, q, _, _ in ac[:n]])
        assert [r[0] for r in res] == add[:n] and all(r == [r[0]] * 4 for r in res)


def test_acc_madd_invariant_is_inductive(dev):
    """x29_acc_madd_tp from worst-case representatives of the accumulator
    (X up to the largest value below 16p, Y + 7p, ZZ / ZZZ + p), then 64
    further additions on each output: the invariant of curve29.h:82 and the
    affine sum after every step, the exceptional branch and its flags when
    the point is the accumulator or its negative"""
    rnd = random.Random(29)
    accs = [fv.madd_start(i, rnd) for i in range(96)]
    top = [0.0, 0.0]
    branches = set()
    for step in range(65):
        n = len(accs)
        accs, st = fv.madd_step(dev.h, accs, step, rnd)
        top = [max(top[0], st[0]), max(top[1], st[1])]
        if len(accs) < n:
            branches.add("inf")
        # cancelled accumulators restart from a fresh worst-case representative
        accs += [fv.madd_start(step + 5 * i, rnd) for i in range(n - len(accs))]
    assert "inf" in branches
    print(f"x29_acc_madd_tp maxima over the chain: X3 {top[0]:.2f}p, Y3 {top[1]:.2f}p")


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("want_y", [1, 0], ids=["level", "last"])
@pytest.mark.parametrize("q4", [1, 0], ids=["q4", "lane"])
@pytest.mark.parametrize("pattern", fv.FOLD_PATTERNS)
def test_msm_fold(dev, pattern, q4, want_y, batch):
    for m in fv.FOLD_M:
        fv.check_fold(dev.h, q4, want_y, batch, m, pattern, 1000 * m + 10 * batch + q4)


def test_msm_fold_rejects_bad_arguments(dev):
    import ctypes as C
    L = fv.lib()
    w = (C.c_uint32 * (32 * 4))()
    ok = dict(q4=1, A=w, Y=w, m=2, batch=1, istride=2, want_y=1, A_out=w, Y_out=w)

    def call(**kw):
        a = dict(ok, **kw)
        return L.qg_selftest_msm_fold(dev.h, a["q4"], a["A"], a["Y"], a["m"], a["batch"], a["istride"],
                                      a["want_y"], a["A_out"], a["Y_out"])
    for bad in (dict(A=None), dict(Y=None), dict(A_out=None), dict(Y_out=None), dict(m=0), dict(m=65537),
                dict(batch=0), dict(batch=17), dict(istride=1), dict(istride=65537)):
        assert call(**bad) == fv.QG_ERR_INVALID, bad
    assert call(want_y=0, Y_out=None) == 0  # all-zero words: infinities in, infinity out
