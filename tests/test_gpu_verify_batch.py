"""Batched KZG verification with the fold on the device
(qg_kzg_verify_batch_dev: one-shot bases, L by qg_msm_g1 over all 2n + 1 of
them, R by qg_msm_g1_at over the slice [n, 2n)) against the host fold.

The claims are fabricated valid with the trapdoor: C = c g1 opened at x to y
has pi = ((c - y) / (tau - x)) g1.  One list of 257 serves every test; the
sets are its prefixes: n = 1, 2, 3 (the smallest MSMs: 3, 5 and 7 bases), 64
and 257 (2n + 1 = 129 and 515 bases: more than one MSM tile, odd sizes, and an
R slice that starts at an odd base offset).  Claim 1 has the identity
commitment (c = 0), claim 2 the identity proof (c = y), so every set but the
first folds identity bases."""
import random

import pytest

import pairing_oracle as po
import quill_oracle as o
import verify_batch_restatement as vb

pytestmark = pytest.mark.gpu
R = o.R_MOD
TAU = 0x48595045524C4F4E4B
SEED = bytes(range(32, 64))
SIZES = [1, 2, 3, 64, 257]
UNSUPPORTED = -4


def _q():
    import quill_amd
    return quill_amd


@pytest.fixture(scope="module")
def vk():
    return _q().KZG.verifier(tau=TAU)


@pytest.fixture(scope="module")
def claims():
    """257 valid claims; c_i and k_i = (c_i - y_i)/(tau - x_i) walk arithmetic
    progressions of full-size scalars, so each point costs one group addition"""
    rnd = random.Random(0xBA7C4)
    c0, dc, k0, dk = (rnd.randrange(1, R) for _ in range(4))
    Cp, Dc = po.g1_mul(po.G1_GEN, c0), po.g1_mul(po.G1_GEN, dc)
    Kp, Dk = po.g1_mul(po.G1_GEN, k0), po.g1_mul(po.G1_GEN, dk)
    out = []
    for i in range(max(SIZES)):
        c, k, x = (c0 + i * dc) % R, (k0 + i * dk) % R, rnd.randrange(R)
        if i == 1:    # identity commitment: the zero polynomial's, opened to y != 0
            out.append((None, x, (-k * (TAU - x)) % R, Kp))
        elif i == 2:  # identity proof: a constant polynomial, y = c
            out.append((Cp, x, c, None))
        else:
            out.append((Cp, x, (c - k * (TAU - x)) % R, Kp))
        Cp, Kp = po.g1_add(Cp, Dc), po.g1_add(Kp, Dk)
    okzg = o.KZG(1, TAU, points=[])
    for Cm, x, y, pi in out[:8] + out[-2:]:
        assert okzg.verify(Cm, (x, y, pi))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_device_fold_equals_host_fold(dev, vk, claims, n):
    q = _q()
    cl = claims[:n]
    for seed in (None, SEED):
        rc_h, Lh, Rh = vb.call_fold(q, vk, cl, seed)
        rc_d, Ld, Rd = vb.call_fold(q, vk, cl, seed, dev)
        assert rc_h == 0 and rc_d == 0
        assert (Ld, Rd) == (Lh, Rh)
        if n <= 3:
            assert (Ld, Rd) == vb.fold(cl, seed)
        assert vb.call_verify(q, vk, cl, seed) == (0, 1, vb.UNTOUCHED)
        assert vb.call_verify(q, vk, cl, seed, dev) == (0, 1, vb.UNTOUCHED)


def test_device_fold_of_identities_and_empty(dev, vk, claims):
    q = _q()
    for cl in ([], [claims[1]], [claims[2]], [claims[2], claims[2]], [claims[1], claims[2]],
               [claims[0], claims[0], claims[5], claims[0]]):
        assert vb.call_fold(q, vk, cl, None, dev) == vb.call_fold(q, vk, cl)
        assert vb.call_verify(q, vk, cl, None, dev) == (0, 1, vb.UNTOUCHED)
    # all-identity set: the fold is the identity on both sides
    zero = (None, 5, 0, None)
    assert vb.call_fold(q, vk, [zero, zero], None, dev) == (0, None, None)
    # off the curve: refused before any device work
    Cm, x, y, pi = claims[0]
    bad = ((Cm[0], (Cm[1] + 1) % po.P), x, y, pi)
    assert vb.call_verify(q, vk, [claims[3], bad], None, dev)[0] == -1


def _with_y(claim, dy):
    Cm, x, y, pi = claim
    return (Cm, x, (y + dy) % R, pi)


@pytest.mark.parametrize("case", ["first", "last", "cancelling pair"])
def test_device_path_rejects_with_the_hosts_first_bad(dev, vk, claims, case):
    q = _q()
    n = 64
    cl = list(claims[:n])
    if case == "first":
        cl[0], want = _with_y(cl[0], 1), 0
    elif case == "last":
        cl[n - 1], want = _with_y(cl[n - 1], 1), n - 1
    else:  # passes with equal weights (tests/test_verify_batch.py restates that)
        cl[4], cl[9], want = _with_y(cl[4], 77), _with_y(cl[9], -77), 4
        assert vb.fold(cl[:10], rho=[1] * 10) == vb.fold(claims[:10], rho=[1] * 10)
    host = vb.call_verify(q, vk, cl)
    assert host == (0, 0, want)
    assert vb.call_verify(q, vk, cl, None, dev) == host
    assert vb.call_fold(q, vk, cl, None, dev) == vb.call_fold(q, vk, cl)


@pytest.mark.parametrize("rows,which", [(8, ("fib", "mod")), (64, ("mod", "fib"))])
def test_device_proved_hyperplonk_verifies_batched(dev, rows, which):
    from test_gpu_hyperplonk import _device_setup
    pcs, hp, ws = _device_setup(dev, rows, which)
    proof = hp.prove(pcs, ws)
    final = hp.last_transcript.state
    assert proof.verify(hp.to_vk(), pcs, batch=True, dev=dev).state == final
    assert proof.verify(hp.to_vk(), pcs, batch=True).state == final
    # the view by hand, with a seed of the verifier's own
    view = pcs.deferring(dev, seed=SEED)
    from quill_amd.proof import _hyperplonk_verify
    assert _hyperplonk_verify(proof, hp.to_vk(), view).state == final
    assert len(view.claims) >= 4 * 7 * len(which)
    view.check()
    op = proof.trace_proofs[1].openings_zero_check[1].poly_opening_inv
    op.proof = po.g1_add(op.proof, po.G1_GEN)
    with pytest.raises(ValueError, match=r"Zero check opening verification failed \(trace 1 "
                                         r"zero-check opening 1, poly_opening_inv; batched claim"):
        proof.verify(hp.to_vk(), pcs, batch=True, dev=dev)


def test_sharded_context_is_unsupported(vk, claims):
    q = _q()
    lb = q.lib()
    group = q.Device.loopback_group(2)
    d = q.Device(0)
    d.attach_loopback(group, 0)
    assert d.comm_info()["sharded"]
    for n in (0, 3):
        rc, ok, bad = vb.call_verify(q, vk, claims[:n], None, d)
        assert (rc, bad) == (UNSUPPORTED, vb.UNTOUCHED)
        assert b"sharded" in lb.qg_last_error(d.h)
        assert vb.call_fold(q, vk, claims[:n], None, d)[0] == UNSUPPORTED
    view = vk.deferring(d)
    Cm, x, y, pi = claims[0]
    view.verify_univariate(Cm, q.KZGOpeningProof(x, y, pi))
    with pytest.raises(q.QuillGpuError) as e:
        view.check()
    assert e.value.code == UNSUPPORTED and "sharded" in str(e.value)
    d.close()
    lb.qg_loopback_destroy(group)
