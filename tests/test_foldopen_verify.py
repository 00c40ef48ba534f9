"""The folded ML opening on the CPU (no GPU needed: the two verifiers, the
pairing and the transcript are host code).

  * the restatement (tests/foldopen_restatement.py) accepts its own proofs and
    ends in the prover's transcript state;
  * qg_mle_verify_folded accepts them with real pairings, in the same state;
  * qg_mle_verify_folded_defer followed by qg_kzg_verify_batch accepts;
  * both reject a tamper of every field, a (y_poly + d, y_s - d / gamma) pair
    that leaves the folded value unchanged, and a wrong commitment;
  * serialize -> deserialize is the identity, standalone and inside a
    MultisetEqualityProof with opening=; truncated input raises; the default
    decoder refuses folded bytes or leaves trailing bytes."""
import copy
import random

import pytest

import foldopen_restatement as fo
import quill_oracle as o

R = o.R_MOD
TAU = 0x48595045524C4F4E4B
DOMAIN = b"foldopen_verify"
NVS = (1, 2, 4)


def _q():
    import quill_amd
    return quill_amd


@pytest.fixture(scope="module")
def vk():
    return _q().KZG.verifier(tau=TAU)


_CACHE = {}


def _case(nv):
    """(kzg, commitment, proof, state before, prover's final state), proven once"""
    if nv not in _CACHE:
        rnd = random.Random(0xF01D + nv)
        poly = [rnd.randrange(R) for _ in range(1 << nv)]
        point = [rnd.randrange(R) for _ in range(nv)]
        kzg = o.KZG(1 << nv, TAU, points=[])
        t = o.Transcript(DOMAIN)
        t.append_g1(kzg.commit(poly))
        before = t.clone()
        proof = fo.prove(poly, point, kzg, t)
        assert proof["evaluation"] == o.mle_evaluate(poly, point)
        _CACHE[nv] = (kzg, kzg.commit(poly), proof, before, t.state)
    return _CACHE[nv]


def _restated(nv, proof, comm):
    kzg, _, _, before, _ = _case(nv)
    t = before.clone()
    return fo.verify(proof, comm, kzg, t), t.state


def _product(vk, nv, proof, comm, defer):
    """(verdict, final state) of the product's verifier; defer: the two claims
    through a deferring view and its one pairing check"""
    q = _q()
    _, _, _, before, _ = _case(nv)
    t = q.Transcript(DOMAIN)
    t.state = before.state
    p = fo.to_product(q, proof)
    if not defer:
        return p.verify(comm, vk, t), t.state
    view = vk.deferring()
    ok = p.verify(comm, view, t)
    assert len(view.claims) == 2
    assert [lbl.split(", ")[1] for lbl, _ in view.claims] == ["folded at r", "folded at 1/r"]
    try:
        view.check()
    except ValueError:
        ok = False
    return ok, t.state


def tampers(nv):
    _, comm, proof, before, _ = _case(nv)
    out = []

    def add(name, edit):
        p = copy.deepcopy(proof)
        edit(p)
        out.append((name, p, comm))

    def point(p):
        p["point"][0] = (p["point"][0] + 1) % R
    add("point", point)

    def evaluation(p):
        p["evaluation"] = (p["evaluation"] + 1) % R
    add("evaluation", evaluation)

    def s_comm(p):
        p["s_comm"] = o.g1_add(p["s_comm"], o.G1_GEN)
    add("s_comm", s_comm)
    for i in range(4):
        def y(p, i=i):
            p["y"][i] = (p["y"][i] + 1) % R
        add("y %d" % i, y)
    for name in ("w", "w_inv"):
        def w(p, name=name):
            p[name] = o.g1_add(p[name], o.G1_GEN)
        add(name, w)

    # y_poly + d with y_s - d / gamma under the HONEST gamma: the folded value
    # y0 + gamma y2 looks unchanged, so only the binding of the y before gamma
    # (and the equation) can reject it
    def cancelling(p, j):
        g = fo.gamma_of(proof, before)
        assert g != 0
        d = 0x1234567
        p["y"][j] = (p["y"][j] + d) % R
        p["y"][2 + j] = (p["y"][2 + j] - d * o.fr_inv(g)) % R
        assert (p["y"][j] + g * p["y"][2 + j]) % R == (proof["y"][j] + g * proof["y"][2 + j]) % R
    add("cancelling pair at r", lambda p: cancelling(p, 0))
    add("cancelling pair at 1/r", lambda p: cancelling(p, 1))
    out.append(("wrong commitment", copy.deepcopy(proof), o.g1_add(comm, o.G1_GEN)))
    return out


# ---------------------------------------------------------------- acceptance
@pytest.mark.parametrize("nv", NVS)
def test_restatement_accepts_its_own_proofs(nv):
    _, comm, proof, _, final = _case(nv)
    assert _restated(nv, proof, comm) == (True, final)


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("defer", [False, True], ids=["sequential", "deferred"])
def test_product_verifier_accepts(vk, nv, defer):
    _, comm, proof, _, final = _case(nv)
    assert _product(vk, nv, proof, comm, defer) == (True, final)


def test_zero_polynomial(vk):
    """L_h = 0: identity commitments, all y 0; both verifiers accept"""
    kzg = o.KZG(4, TAU, points=[])
    t = o.Transcript(DOMAIN)
    before = t.clone()
    proof = fo.prove([0, 0, 0, 0], [5, 7], kzg, t)
    assert proof["y"] == [0] * 4 and proof["w"] is None and proof["w_inv"] is None
    assert proof["s_comm"] is None
    t2 = before.clone()
    assert fo.verify(proof, None, kzg, t2) and t2.state == t.state
    q = _q()
    for view in (vk, vk.deferring()):
        tq = q.Transcript(DOMAIN)
        assert fo.to_product(q, proof).verify(None, view, tq) and tq.state == t.state
        if view is not vk:
            view.check()


# ---------------------------------------------------------------- rejection
@pytest.mark.parametrize("nv", NVS)
def test_restatement_rejects_every_tamper(nv):
    for name, p, comm in tampers(nv):
        ok, _ = _restated(nv, p, comm)
        assert not ok, name


@pytest.mark.parametrize("nv", NVS)
@pytest.mark.parametrize("defer", [False, True], ids=["sequential", "deferred"])
def test_product_verifier_rejects_every_tamper(vk, nv, defer):
    for name, p, comm in tampers(nv):
        ok, state = _product(vk, nv, p, comm, defer)
        assert not ok, name
        # the transcript advances whatever the verdict, as the restatement's
        assert state == _restated(nv, p, comm)[1], name


def test_point_off_the_curve_is_invalid(vk):
    q = _q()
    _, comm, proof, _, _ = _case(2)
    for name in ("w", "w_inv", "s_comm"):
        p = copy.deepcopy(proof)
        p[name] = (p[name][0], (p[name][1] + 1) % o.P_MOD)
        for view in (vk, vk.deferring()):
            with pytest.raises(q.QuillGpuError) as e:
                fo.to_product(q, p).verify(comm, view, q.Transcript(DOMAIN))
            assert e.value.code == -1, name


# ---------------------------------------------------------------- wire format
@pytest.mark.parametrize("nv", NVS)
def test_serialize_roundtrip(nv):
    q = _q()
    _, _, proof, _, _ = _case(nv)
    p = fo.to_product(q, proof)
    b = q.serialize(p)
    assert len(b) == 8 + 32 * nv + 32 + 64 + 256
    assert q.deserialize(q.FoldedMLEvalProof, b) == p
    assert q.deserialize(q.MLEvalProof, b, opening=q.FoldedMLEvalProof) == p
    for cut in (0, 1, len(b) // 2, len(b) - 1):
        with pytest.raises(ValueError):
            q.deserialize(q.FoldedMLEvalProof, b[:cut])
    with pytest.raises(ValueError):
        q.deserialize(q.FoldedMLEvalProof, b + b"\0")
    # the default decoder reads four KZG openings: folded bytes are too short
    with pytest.raises(ValueError):
        q.deserialize(q.MLEvalProof, b)
    with pytest.raises(TypeError):
        q.deserialize(q.MLEvalProof, b, opening=q.KZGOpeningProof)


def test_serialize_inside_a_composite_proof():
    q = _q()
    pl, pr = (fo.to_product(q, _case(nv)[2]) for nv in (2, 4))
    sc = q.SumcheckProof(2, 5, [[1, 2, 3], [4, 5]])
    m = q.MultisetEqualityProof(o.G1_GEN, None, sc, pl, pr)
    b = q.serialize(m)
    assert q.deserialize(q.MultisetEqualityProof, b, opening=q.FoldedMLEvalProof) == m
    with pytest.raises(ValueError):  # refused, or trailing bytes left
        q.deserialize(q.MultisetEqualityProof, b)
    with pytest.raises(ValueError):
        q.deserialize(q.MultisetEqualityProof, b[:-1], opening=q.FoldedMLEvalProof)
    # a default proof still decodes by default, and not as folded
    okzg = o.KZG(4, TAU, points=[])
    op = o.MLEvalProof.prove([1, 2, 3, 4], [5, 6], okzg, o.Transcript(DOMAIN))
    plain = q.MLEvalProof(op.evaluation_point, op.evaluation, op.s_comm,
                          *[q.KZGOpeningProof(*x) for x in (op.poly_opening, op.poly_opening_inv,
                                                            op.s_opening, op.s_opening_inv)])
    pb = q.serialize(plain)
    assert q.deserialize(q.MLEvalProof, pb) == plain
    with pytest.raises(ValueError):
        q.deserialize(q.MLEvalProof, pb, opening=q.FoldedMLEvalProof)
