"""InnerProductProof::prove on the device (qg_ipa_prove / qg_ipa_prove_dev,
ipa.rs:59-112) against the restatement in tests/ipa_restatement.py: the inner
product, s_comm, all six (x, y, proof) and the transcript state, bit for bit.

Sizes: the serial scan (<= SH_B = 32) and the first length past it; 2M - 1 =
1025 (a two-pass NTT); 1025 coefficients = 33 chunks (the scan recursion two
levels deep); zero tails (trimmed lengths); an all-zero operand (S empty,
identity commitments); and 2M - 1 > 2^17 (three NTT passes), which is checked
by the verifiers instead of the O(n^2) restated prover.  The single-job
route (default, QG_IPA_PAIRED=0) and the paired suffix-Horner kernels
(QG_IPA_PAIRED=1) must give identical proofs.  The switches are read per call,
so the tests toggle them in-process."""
import contextlib
import ctypes as C
import os
import random

import pytest

import ipa_restatement as ipa
import quill_oracle as o

pytestmark = pytest.mark.gpu
R = o.R_MOD
TAU = 0x495041474F4C44
DOMAIN = b"gpu-ipa"
MAXDEG = 1 << 12


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name)
        else:
            os.environ[name] = old


def vec(n, seed, live=None):
    rnd = random.Random(seed)
    live = n if live is None else live
    return [rnd.randrange(1, R) if i < live else 0 for i in range(n)]


# name -> (f, g)
CASES = {
    "3x3": (vec(3, 1), vec(3, 2)),
    "3x2": (vec(3, 3), vec(2, 4)),
    "2x3": (vec(2, 5), vec(3, 6)),
    "1x1": (vec(1, 7), vec(1, 8)),
    "3x0": (vec(3, 9), []),
    "33x33": (vec(33, 10), vec(33, 11)),        # first length past the serial scan
    "33x2": (vec(33, 12), vec(2, 13)),          # serial and chunked jobs in one call
    "513x300": (vec(513, 14), vec(300, 15)),    # 2M - 1 = 1025: a two-pass NTT
    "1025x1025": (vec(1025, 16), vec(1025, 17)),  # 33 chunks: the recursion two levels deep
    "64x64_f40": (vec(64, 18, live=40), vec(64, 19)),
    "64x64_g0": (vec(64, 20), [0] * 64),        # S empty, identity commitments
}
PARITY = ["3x3", "3x2", "2x3", "1x1", "3x0", "33x33", "513x300", "1025x1025", "64x64_f40",
          "64x64_g0"]
_restated = {}


def restated(name):
    """(proof tuple, final transcript state) of the restated prover, computed once"""
    if name not in _restated:
        f, g = CASES[name]
        t = o.Transcript(DOMAIN)
        _restated[name] = (ipa.prove(f, g, o.KZG(MAXDEG, TAU, points=[]), t), t.state)
    return _restated[name]


@pytest.fixture(scope="module")
def kzg(dev):
    """the SRS, after one larger ML opening: the NTT scratch (shared with the
    S polynomial of the inner-product argument) then holds stale data"""
    from quill_amd import KZG, DeviceVec, Transcript
    k = KZG.trusted_setup(MAXDEG, TAU, dev)
    v = DeviceVec(dev, 1 << 12).fill_random(0x57A1E)
    k.open_dev(v, len(v), vec(12, 21), Transcript(b"stale"))
    v.close()
    yield k
    k.close()


def prove(kzg, f, g, on_device=False):
    from quill_amd import DeviceVec, InnerProductProof, Transcript
    t = Transcript(DOMAIN)
    if on_device:
        # (an empty operand: a one-entry buffer, stated length 0)
        df, dg = DeviceVec.from_list(kzg.dev, f or [0]), DeviceVec.from_list(kzg.dev, g or [0])
        p = _prove_dev(kzg, df, len(f), dg, len(g), t)
        df.close()
        dg.close()
    else:
        p = InnerProductProof.prove(f, g, kzg, t)
    return p, t.state


def _prove_dev(kzg, df, nf, dg, ng, t):
    """qg_ipa_prove_dev on the first nf / ng entries"""
    import quill_amd as q
    from quill_amd._lib import IpaProof, check, lib
    out = IpaProof()
    check(lib().qg_ipa_prove_dev(kzg.dev.h, kzg.srs.h, df.h, nf, dg.h, ng, t.c_state(),
                                 C.byref(out)), kzg.dev.h)
    from quill_amd.pcs import _IPA_OPENINGS, _opening
    from quill_amd.field import fr_from_mont_limbs, g1_from_abi
    return q.InnerProductProof(fr_from_mont_limbs(list(out.inner_product)),
                               g1_from_abi(out.s_comm_xy, out.s_comm_inf),
                               *[_opening(getattr(out, n)) for n in _IPA_OPENINGS])


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("name", PARITY)
def test_parity_with_the_restatement(dev, kzg, name):
    f, g = CASES[name]
    want, want_state = restated(name)
    f0 = dev.counter("open_check_failures")
    got, state = prove(kzg, f, g)
    assert got.inner_product == want[0]
    assert got.s_comm == want[1]
    for nm, w in zip(ipa.OPENINGS, want[2:]):
        op = getattr(got, nm)
        assert (op.x, op.y, op.proof) == w, nm
    assert state == want_state
    assert dev.counter("open_check_failures") == f0


def test_reference_kats(kzg):
    """ipa.rs:230, :273"""
    assert prove(kzg, [1, 2, 3], [4, 5, 6])[0].inner_product == 32
    assert prove(kzg, [1, 2, 3], [4, 5])[0].inner_product == 14
    assert prove(kzg, [1, 2], [4, 5, 6])[0].inner_product == 14


def test_empty_s_has_identity_commitments(kzg):
    for name in ("1x1", "3x0", "64x64_g0"):
        p, _ = prove(kzg, *CASES[name])
        assert p.s_comm is None
        assert (p.s_opening.y, p.s_opening.proof) == (0, None)
        assert (p.s_opening_inv.y, p.s_opening_inv.proof) == (0, None)


def test_device_entry_equals_host_entry(kzg):
    f, g = CASES["513x300"]
    assert prove(kzg, f, g, on_device=True) == prove(kzg, f, g)
    want, want_state = restated("513x300")
    got, state = prove(kzg, f, g, on_device=True)
    assert (ipa.from_product(got), state) == (want, want_state)


def test_device_entry_uses_the_stated_lengths(kzg):
    """the first nf / ng entries of larger buffers"""
    from quill_amd import DeviceVec, Transcript
    f, g = CASES["513x300"]
    df = DeviceVec.from_list(kzg.dev, f + vec(100, 30))
    dg = DeviceVec.from_list(kzg.dev, g + vec(7, 31))
    t = Transcript(DOMAIN)
    got = _prove_dev(kzg, df, len(f), dg, len(g), t)
    df.close()
    dg.close()
    assert (ipa.from_product(got), t.state) == restated("513x300")


@pytest.mark.parametrize("name", ["1025x1025", "33x2"])
def test_paired_and_single_jobs_give_identical_proofs(kzg, name):
    f, g = CASES[name]
    with env("QG_IPA_PAIRED", "1"):
        paired = prove(kzg, f, g)
    with env("QG_IPA_PAIRED", "0"):
        single = prove(kzg, f, g)
    assert paired == single == prove(kzg, f, g)
    assert (ipa.from_product(paired[0]), paired[1]) == restated(name)


# ---------------------------------------------------------------- three NTT passes
def test_three_ntt_passes(dev):
    """nf = 70000, ng = 65537: 2M - 1 > 2^17.  The restated prover is O(n^2);
    the verifiers are not: the restated one (trapdoor KZG) and qg_ipa_verify
    (pairings) accept, in the prover's final transcript state."""
    import quill_amd as q
    nf, ng = 70000, 65537
    f, g = vec(nf, 40), vec(ng, 41)
    kz = q.KZG.trusted_setup(nf, TAU, dev)
    df, dg = q.DeviceVec.from_list(dev, f), q.DeviceVec.from_list(dev, g)
    t = q.Transcript(DOMAIN)
    proof = q.InnerProductProof.prove(df, dg, kz, t)
    df.close()
    dg.close()
    assert proof.inner_product == sum(a * b for a, b in zip(f, g)) % R
    okzg = o.KZG(nf, TAU, points=[])
    c1, c2 = okzg.commit(f), okzg.commit(g)
    vt = o.Transcript(DOMAIN)
    assert ipa.verify(ipa.from_product(proof), c1, c2, okzg, vt)
    assert vt.state == t.state
    back = q.deserialize(q.InnerProductProof, q.serialize(proof))
    assert back == proof
    pt = q.Transcript(DOMAIN)
    assert back.verify(c1, c2, kz, pt)
    assert pt.state == t.state
    kz.close()


# ---------------------------------------------------------------- the NTT memo
def test_ntt_memo_is_truthful_after_an_ipa_call(dev, kzg):
    """open_dev(vec); an IPA proof of two OTHER vectors of the same size (it
    transforms f into the scratch that held vec's transform); open_dev(vec,
    unchanged=True) must not reuse what that scratch holds now"""
    from quill_amd import DeviceVec, InnerProductProof, Transcript
    n = 1 << 10
    v = DeviceVec(dev, n).fill_random(0xAA01)
    a = DeviceVec(dev, n).fill_random(0xAA02)
    b = DeviceVec(dev, n).fill_random(0xAA03)
    pt = vec(10, 50)
    t1 = Transcript(b"memo")
    first = kzg.open_dev(v, n, pt, t1)
    InnerProductProof.prove(a, b, kzg, Transcript(DOMAIN))
    t3 = Transcript(b"memo")
    third = kzg.open_dev(v, n, pt, t3, unchanged=True)
    assert third == first and t3.state == t1.state
    for x in (v, a, b):
        x.close()


# ---------------------------------------------------------------- the quotient check
def counters(dev):
    return dev.counter("open_checks"), dev.counter("open_check_failures")


def test_six_quotients_are_counted(dev, kzg):
    c0, f0 = counters(dev)
    prove(kzg, *CASES["3x3"])
    assert counters(dev) == (c0 + 6, f0)
    with env("QG_OPEN_CHECK", "0"):
        assert prove(kzg, *CASES["3x3"])[1] == restated("3x3")[1]
    assert counters(dev) == (c0 + 6, f0)


def test_corrupt_quotient_is_caught_and_named(dev, kzg):
    from quill_amd._lib import QuillGpuError
    f, g = CASES["33x33"]
    c0, f0 = counters(dev)
    dev.debug_open_fault(2, 5)
    with pytest.raises(QuillGpuError) as e:
        prove(kzg, f, g)
    assert e.value.code == -5
    assert "Polynomial division failed" in str(e.value)
    assert "(f at r)" in str(e.value), str(e.value)
    c1, f1 = counters(dev)
    assert f1 > f0 and c1 == c0 + 6
    # one-shot: the next call is clean
    got, state = prove(kzg, f, g)
    assert (ipa.from_product(got), state) == restated("33x33")
    assert dev.counter("open_check_failures") == f1


def test_corrupt_quotient_of_g_is_caught_and_named(dev, kzg):
    """f of one coefficient has no quotient coefficients, so the fault lands in
    the first non-empty quotient: g's at r.  (No shape sends it to S's: when
    neither f nor g has a quotient, both are constants and S is empty.)"""
    from quill_amd._lib import QuillGpuError
    f, g = [5], [7, 11, 13]
    want = prove(kzg, f, g)
    assert want[0].f_opening.proof is None and want[0].s_opening.proof is not None
    dev.debug_open_fault(2, 0)
    with pytest.raises(QuillGpuError) as e:
        prove(kzg, f, g)
    assert e.value.code == -5 and "(g at r)" in str(e.value), str(e.value)
    assert prove(kzg, f, g) == want


def test_short_trim_is_caught(dev, kzg):
    from quill_amd._lib import QuillGpuError
    f, g = CASES["3x3"]
    f0 = dev.counter("open_check_failures")
    dev.debug_open_fault(1, 1)
    with pytest.raises(QuillGpuError) as e:
        prove(kzg, f, g)
    assert e.value.code == -5
    assert dev.counter("open_check_failures") > f0
    got, state = prove(kzg, f, g)
    assert (ipa.from_product(got), state) == restated("3x3")


# ---------------------------------------------------------------- statuses
def test_statuses(dev, kzg):
    import quill_amd as q
    from quill_amd._lib import IpaProof, lib
    from quill_amd.field import fr_array, u64p
    L = lib()
    out = IpaProof()
    st = q.Transcript(DOMAIN).c_state()
    a = fr_array([1, 2, 3])
    da, db = q.DeviceVec.from_list(dev, [1, 2, 3]), q.DeviceVec.from_list(dev, [4, 5, 6])

    def host(ctx=dev.h, srs=kzg.srs.h, f=u64p(a), nf=3, g=u64p(a), ng=3, state=st, o_=out):
        return L.qg_ipa_prove(ctx, srs, f, nf, g, ng, state, C.byref(o_) if o_ else None)

    def devc(ctx=dev.h, srs=kzg.srs.h, f=da.h, nf=3, g=db.h, ng=3, state=st, o_=out):
        return L.qg_ipa_prove_dev(ctx, srs, f, nf, g, ng, state, C.byref(o_) if o_ else None)

    def last(d=dev):
        m = L.qg_last_error(d.h)
        return m.decode() if m else ""

    assert host() == 0 and devc() == 0
    # both lengths 0 (the reference underflows 2 max_len - 1)
    assert host(nf=0, ng=0) == -1 and devc(nf=0, ng=0) == -1
    assert host(f=None, nf=0, g=None, ng=0) == -1
    # one empty operand is a proof
    assert host(f=None, nf=0) == 0 and devc(ng=0) == 0
    # null handles and pointers
    assert host(ctx=None) == -1 and host(srs=None) == -1 and host(f=None) == -1
    assert host(g=None) == -1 and host(state=None) == -1 and host(o_=None) == -1
    assert devc(ctx=None) == -1 and devc(srs=None) == -1 and devc(f=None) == -1
    assert devc(g=None) == -1 and devc(state=None) == -1 and devc(o_=None) == -1
    # a length beyond the buffer
    assert devc(nf=4) == -1 and devc(ng=4) == -1
    # an SRS too short: 17 coefficients, a quotient of 16 against 9 bases
    small = q.KZG.trusted_setup(8, TAU, dev)
    big = fr_array(vec(17, 60))
    assert host(srs=small.srs.h, f=u64p(big), nf=17) == -1
    assert "Polynomial degree exceeds max degree" in last()
    # ... and an S too long: S_k = f_{k+1} g_0, 11 coefficients against 9 bases
    assert host(srs=small.srs.h, f=u64p(fr_array([0] * 11 + [1])), nf=12, g=u64p(a), ng=1) == -1
    assert "Polynomial degree exceeds max degree" in last()
    small.close()
    # a context with a two-rank loopback communicator attached
    group = q.Device.loopback_group(2)
    d2 = q.Device(0)
    d2.attach_loopback(group, 0)
    assert d2.comm_info()["sharded"]
    assert host(ctx=d2.h) == -4
    assert "sharded" in last(d2)
    d2.close()
    L.qg_loopback_destroy(group)
    da.close()
    db.close()
