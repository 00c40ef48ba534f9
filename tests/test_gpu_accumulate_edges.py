"""The edges of the bucket accumulation's loop body (k_msm_accumulate_coop keeps
its accumulator in place on every path: curve29.h x29_acc_start_ip /
x29_acc_madd_ip), forced onto small MSMs with QG_MSM_COOP=1 and compared with
the default loop (k_msm_accumulate<false>) of the same chunk length:

  * the exceptional lanes inside the kernel: a bucket that meets P, P (the
    accumulator is doubled at the second entry of its run), P, -P (it cancels
    to infinity, and the next entry starts a fresh run), a run that ends at
    infinity, infinity bases, and all of these cut by chunk boundaries
    (QG_MSM_ELOG=2: four entries per lane, so the groups of three straddle
    them at every phase and the doubling / cancellation moves to the
    reduction's additions);
  * run starts and partial waves: 1 .. 257 scalars with four and eight entries
    per lane, 12-bit scalars (few, crowded buckets: some lane flushes and
    starts a run at nearly every step) and full-width ones.
"""
import contextlib
import os
import random

import pytest

import quill_oracle as o

pytestmark = pytest.mark.gpu
R = o.R_MOD


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


def both_loops(srs, scal, elog):
    """the MSM by the cooperative loop and by the default loop"""
    out = []
    for coop in ("1", "0"):
        with env(QG_MSM_COOP=coop, QG_MSM_PF="0", QG_MSM_ELOG=elog):
            out.append(srs.msm(scal))
    return out


@pytest.fixture(scope="module")
def exceptional():
    """192 bases from 64 random points P = [t] g, three per point with one
    scalar s per point, so their equal digits meet in one bucket:
      even points  P,  P, -P   doubling at the second entry, then 2Q - Q
      odd points   P, -P,  P   cancellation to infinity, then a fresh start
    and at the end Z, -Z with one scalar (the run ends at infinity), with an
    infinity base after every 50th.  Expected: sum s_j P_j (+ 0)."""
    rnd = random.Random(0xACC)
    bases, scal, want = [], [], None
    for j in range(64):
        P = o.g1_mul(o.G1_GEN, rnd.randrange(1, R))
        s = rnd.randrange(R)
        bases += [P, P, o.g1_neg(P)] if j % 2 == 0 else [P, o.g1_neg(P), P]
        scal += [s, s, s]
        want = o.g1_add(want, o.g1_mul(P, s))
    Z = o.g1_mul(o.G1_GEN, rnd.randrange(1, R))
    s = rnd.randrange(R)
    bases += [Z, o.g1_neg(Z)]
    scal += [s, s]
    for k in range(len(bases) // 50, 0, -1):
        bases.insert(50 * k, None)
        scal.insert(50 * k, rnd.randrange(R))
    return bases, scal, want


@pytest.mark.parametrize("elog", [None, "2", "3"])
def test_doubling_and_cancellation_in_the_loop(dev, exceptional, elog):
    from quill_amd import Srs
    bases, scal, want = exceptional
    assert sum(b is not None for b in bases) == 194
    srs = Srs.upload(dev, bases)
    coop, default = both_loops(srs, scal, elog)
    srs.close()
    assert coop == want
    assert default == want


def test_every_run_cancels(dev):
    """pairs P, -P only: every bucket's run ends at infinity, the sum is 0"""
    from quill_amd import Srs
    rnd = random.Random(0xCA)
    bases, scal = [], []
    for _ in range(40):
        P = o.g1_mul(o.G1_GEN, rnd.randrange(1, R))
        s = rnd.randrange(R)
        bases += [P, o.g1_neg(P)]
        scal += [s, s]
    srs = Srs.upload(dev, bases)
    for elog in (None, "2"):
        assert both_loops(srs, scal, elog) == [None, None]
    srs.close()


_SRS = {}


@pytest.fixture(scope="module")
def srs_of(dev):
    from quill_amd import Srs
    tau = 0x5EED0ACC

    def get(n):
        if n not in _SRS:
            _SRS[n] = Srs.generate(dev, tau, n)
        return _SRS[n], tau
    yield get
    for s in _SRS.values():
        s.close()
    _SRS.clear()


@pytest.mark.parametrize("small", [True, False])
@pytest.mark.parametrize("elog", ["2", "3"])
@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 257])
def test_run_starts_and_partial_waves(srs_of, n, elog, small):
    srs, tau = srs_of(n)
    rnd = random.Random(1000 * n + 10 * int(elog) + small)
    scal = [rnd.randrange(1 << 12) if small else rnd.randrange(R) for _ in range(n)]
    coop, default = both_loops(srs, scal, elog)
    assert coop == default
    assert coop == o.g1_mul(o.G1_GEN, o.poly_eval(scal, tau))
