"""The folded inner-product argument on the CPU (no GPU needed: the two
verifiers, the pairing and the transcript are host code).

  * the restatement (tests/foldipa_restatement.py) accepts its own proofs and
    ends in the prover's transcript state; its fast S equals the oracle's;
  * qg_ipa_verify_folded accepts them with real pairings, in the same state;
  * qg_ipa_verify_folded_defer followed by qg_kzg_verify_batch accepts, with
    exactly 2 claims;
  * both reject a tamper of every field, swapped commitments, the three
    cancelling pairs at r that leave the folded value unchanged (and one at
    1/r), and a proof whose six y are the true values of other polynomials
    (every KZG claim holds) but break the equation; after every rejection the
    transcript state equals the restated verifier's;
  * serialize -> deserialize is the identity, the length is the sum of the
    field encodings and smaller than the plain proof's; truncated input raises."""
import copy
import random

import pytest

import foldipa_restatement as fi
import ipa_restatement as ipa
import quill_oracle as o

R = o.R_MOD
TAU = 0x464F4C44495041
DOMAIN = b"foldipa_verify"
LENS = ((1, 1), (4, 4), (5, 3), (16, 16))
IDS = ["%dx%d" % ln for ln in LENS]


def _q():
    import quill_amd
    return quill_amd


@pytest.fixture(scope="module")
def vk():
    return _q().KZG.verifier(tau=TAU)


_CACHE = {}


def _case(ln):
    """(kzg, (C_f, C_g), proof, state before, prover's final state, (f, g)), proven once"""
    if ln not in _CACHE:
        rnd = random.Random(0xF01D1 + 100 * ln[0] + ln[1])
        f = [rnd.randrange(1, R) for _ in range(ln[0])]
        g = [rnd.randrange(1, R) for _ in range(ln[1])]
        kzg = o.KZG(max(ln), TAU, points=[])
        t = o.Transcript(DOMAIN)
        comms = (kzg.commit(f), kzg.commit(g))
        t.append_g1(comms[0])
        t.append_g1(comms[1])
        before = t.clone()
        proof = fi.prove(f, g, kzg, t)
        assert proof["inner_product"] == sum(a * b for a, b in zip(f, g)) % R
        _CACHE[ln] = (kzg, comms, proof, before, t.state, (f, g))
    return _CACHE[ln]


def _restated(ln, proof, comms):
    kzg, _, _, before, _, _ = _case(ln)
    t = before.clone()
    return fi.verify(proof, comms[0], comms[1], kzg, t), t.state


def _product(vk, ln, proof, comms, defer):
    """(verdict, final state) of the product's verifier; defer: the two claims
    through a deferring view and its one pairing check"""
    q = _q()
    before = _case(ln)[3]
    t = q.Transcript(DOMAIN)
    t.state = before.state
    p = fi.to_product(q, proof)
    if not defer:
        return p.verify(comms[0], comms[1], vk, t), t.state
    view = vk.deferring()
    ok = p.verify(comms[0], comms[1], view, t)
    assert len(view.claims) == 2
    assert [lbl.split(", ")[1] for lbl, _ in view.claims] == ["folded at r", "folded at 1/r"]
    try:
        view.check()
    except ValueError:
        ok = False
    return ok, t.state


def other_polynomials(ln):
    """a proof by a prover who commits and opens S' = S + 1 instead of S: the
    six y are the true values of f, g and S', both quotients are honest for
    f + gamma g + gamma^2 S', so every KZG claim holds against (C_f, C_g,
    s_comm'); only the equation on the six y can reject it"""
    kzg, comms, proof, before, _, (f, g) = _case(ln)
    s_bad = fi.s_polynomial(f, g) or [0]
    s_bad = [(s_bad[0] + 1) % R] + s_bad[1:]
    s_comm = kzg.commit(s_bad)
    t = before.clone()
    t.append_fr(proof["inner_product"])
    t.append_g1(s_comm)
    r = t.draw_field_element()
    r_inv = o.fr_inv(r)
    y = [o.poly_eval(p, x) for p in (f, g, s_bad) for x in (r, r_inv)]
    assert not fi.equation_holds(proof["inner_product"], r, y)
    for v in y:
        t.append_fr(v)
    gamma = t.draw_field_element()
    h = fi.fold((f, g, s_bad), gamma)
    w, yh = fi.quotient_commit(h, r, kzg)
    w_inv, yh_inv = fi.quotient_commit(h, r_inv, kzg)
    g2 = gamma * gamma % R
    c_h = o.g1_add(o.g1_add(comms[0], o.g1_mul(comms[1], gamma)), o.g1_mul(s_comm, g2))
    assert kzg.verify(c_h, (r, yh, w)) and kzg.verify(c_h, (r_inv, yh_inv, w_inv))
    assert yh == (y[0] + gamma * y[2] + g2 * y[4]) % R
    return {"inner_product": proof["inner_product"], "s_comm": s_comm, "y": y, "w": w,
            "w_inv": w_inv}


def tampers(ln):
    _, comms, proof, before, _, _ = _case(ln)
    out = []

    def add(name, edit):
        p = copy.deepcopy(proof)
        edit(p)
        out.append((name, p, comms))

    def inner_product(p):
        p["inner_product"] = (p["inner_product"] + 1) % R
    add("inner_product", inner_product)
    for name in ("s_comm", "w", "w_inv"):
        def pt(p, name=name):
            p[name] = o.g1_add(p[name], o.G1_GEN)
        add(name, pt)
    for i in range(6):
        def y(p, i=i):
            p["y"][i] = (p["y"][i] + 1) % R
        add("y %d" % i, y)

    # y_a + d with y_b - d / gamma^k under the HONEST gamma (k: how many powers
    # of gamma separate the two): the folded value looks unchanged, so only the
    # binding of the six y before gamma (and the equation) can reject it
    def cancelling(p, a, b, at):
        g = fi.gamma_of(proof, before)
        assert g != 0
        d, k = 0x1234567, (b - a) // 2
        p["y"][a] = (p["y"][a] + d) % R
        p["y"][b] = (p["y"][b] - d * o.fr_inv(pow(g, k, R))) % R

        def folded(y):
            return (y[at] + g * y[2 + at] + g * g * y[4 + at]) % R
        assert folded(p["y"]) == folded(proof["y"])
    add("cancelling (y_f, y_g) at r", lambda p: cancelling(p, 0, 2, 0))
    add("cancelling (y_g, y_S) at r", lambda p: cancelling(p, 2, 4, 0))
    add("cancelling (y_f, y_S) at r", lambda p: cancelling(p, 0, 4, 0))
    add("cancelling (y_f, y_g) at 1/r", lambda p: cancelling(p, 1, 3, 1))
    out.append(("swapped commitments", copy.deepcopy(proof), (comms[1], comms[0])))
    out.append(("the values of other polynomials", other_polynomials(ln), comms))
    return out


# ---------------------------------------------------------------- acceptance
@pytest.mark.parametrize("ln", LENS, ids=IDS)
def test_restatement_accepts_its_own_proofs(ln):
    _, comms, proof, _, final, (f, g) = _case(ln)
    assert _restated(ln, proof, comms) == (True, final)
    assert fi.s_polynomial(f, g) == o.compute_s_polynomial(f, g)
    if ln == (1, 1):  # S empty, quotients empty
        assert proof["s_comm"] is None and proof["w"] is None and proof["w_inv"] is None
        assert proof["y"] == [f[0], f[0], g[0], g[0], 0, 0]


@pytest.mark.parametrize("ln", LENS, ids=IDS)
@pytest.mark.parametrize("defer", [False, True], ids=["sequential", "deferred"])
def test_product_verifier_accepts(vk, ln, defer):
    _, comms, proof, _, final, _ = _case(ln)
    assert _product(vk, ln, proof, comms, defer) == (True, final)


def test_restatement_agrees_with_the_plain_argument():
    """the first half is InnerProductProof::prove's: same inner_product, s_comm
    and the six y of the plain proof's openings"""
    kzg, _, proof, before, _, (f, g) = _case((5, 3))
    plain = ipa.prove(f, g, kzg, before.clone())
    assert (plain[0], plain[1]) == (proof["inner_product"], proof["s_comm"])
    assert [op[1] for op in plain[2:]] == proof["y"]


# ---------------------------------------------------------------- rejection
@pytest.mark.parametrize("ln", LENS, ids=IDS)
def test_restatement_rejects_every_tamper(ln):
    for name, p, comms in tampers(ln):
        ok, _ = _restated(ln, p, comms)
        assert not ok, name


@pytest.mark.parametrize("ln", LENS, ids=IDS)
@pytest.mark.parametrize("defer", [False, True], ids=["sequential", "deferred"])
def test_product_verifier_rejects_every_tamper(vk, ln, defer):
    for name, p, comms in tampers(ln):
        ok, state = _product(vk, ln, p, comms, defer)
        assert not ok, name
        # the transcript advances whatever the verdict, as the restatement's
        assert state == _restated(ln, p, comms)[1], name


def test_point_off_the_curve_is_invalid(vk):
    q = _q()
    _, comms, proof, _, _, _ = _case((4, 4))
    for name in ("w", "w_inv", "s_comm"):
        p = copy.deepcopy(proof)
        p[name] = (p[name][0], (p[name][1] + 1) % o.P_MOD)
        for view in (vk, vk.deferring()):
            with pytest.raises(q.QuillGpuError) as e:
                fi.to_product(q, p).verify(comms[0], comms[1], view, q.Transcript(DOMAIN))
            assert e.value.code == -1, name


# ---------------------------------------------------------------- wire format
@pytest.mark.parametrize("ln", LENS, ids=IDS)
def test_serialize_roundtrip(ln):
    q = _q()
    kzg, _, proof, before, _, (f, g) = _case(ln)
    p = fi.to_product(q, proof)
    b = q.serialize(p)
    # inner_product, s_comm, six y, w, w_inv
    assert len(b) == 32 + 64 + 6 * 32 + 2 * 64
    assert q.deserialize(q.FoldedInnerProductProof, b) == p
    plain = ipa.to_product(q, ipa.prove(f, g, kzg, before.clone()))
    assert len(b) < len(q.serialize(plain))
    for cut in (0, 1, len(b) // 2, len(b) - 1):
        with pytest.raises(ValueError):
            q.deserialize(q.FoldedInnerProductProof, b[:cut])
    with pytest.raises(ValueError):
        q.deserialize(q.FoldedInnerProductProof, b + b"\0")
    # the plain decoder reads six KZG openings: folded bytes are too short
    with pytest.raises(ValueError):
        q.deserialize(q.InnerProductProof, b)
