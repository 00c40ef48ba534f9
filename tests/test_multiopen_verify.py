"""The multi-point batch opening on the CPU (no GPU needed: the product's
verifier, qg_g1_lincomb, the pairing and the transcript are host code).

  * the restatement (tests/multiopen_restatement.py) accepts its own proofs and
    ends in the prover's transcript state;
  * quill_amd.MultiOpenProof.verify accepts the same proofs with real pairing
    checks and ends in the same state;
  * both reject every tampered field with the message the protocol names;
  * qg_g1_lincomb equals the oracle's naive MSM, identity cases included;
  * serialize -> deserialize is the identity; truncated input raises."""
import copy
import ctypes as C
import random

import pytest

import multiopen_restatement as mo
import quill_oracle as o

R = o.R_MOD
TAU = 0x48595045524C4F4E4B
DOMAIN = b"multiopen_verify"
CASES = [(n, P, k) for n in (1, 2, 4) for P, k in ((1, 1), (1, 3), (3, 5))]

SHAPE = "Multi-open proof shape mismatch"
SUM = "Multi-open claimed sum mismatch"
ROUND = "Sumcheck polynomial does not sum to previous value"
FINAL = "Multi-open final evaluation mismatch"
OPENING = "Multi-open opening verification failed"


def _q():
    import quill_amd
    return quill_amd


_CACHE = {}


def _case(n, P, k):
    """(polys, claims, kzg, commitments, proof, prover's final state), proven once"""
    if (n, P, k) not in _CACHE:
        polys, claims = mo.make_case(n, P, k)
        kzg = o.KZG(1 << n, TAU, points=[])
        t = o.Transcript(DOMAIN)
        proof = mo.prove(polys, claims, kzg, t)
        _CACHE[(n, P, k)] = (polys, claims, kzg, [kzg.commit(f) for f in polys], proof, t.state)
    return _CACHE[(n, P, k)]


def _pad3(rp):
    return list(rp) + [0] * (3 - len(rp))


def tampers(proof, comms, claims):
    """(name, proof, commitments, claims, expected message) for every tamper"""
    out = []

    def add(name, msg, edit=None, comms_=None, claims_=None):
        p = copy.deepcopy(proof)
        if edit:
            edit(p)
        out.append((name, p, comms_ or comms, claims_ or claims, msg))

    for i in range(len(proof["evaluations"])):
        def ev(p, i=i):
            p["evaluations"][i] = (p["evaluations"][i] + 1) % R
        add(f"evaluation {i}", SUM, ev)

    def claimed(p):
        p["sumcheck"][1] = (p["sumcheck"][1] + 1) % R
    add("claimed sum", SUM, claimed)

    def coeff(p):
        rp = _pad3(p["sumcheck"][2][0])
        rp[1] = (rp[1] + 1) % R
        p["sumcheck"][2][0] = rp
    add("round coefficient", ROUND, coeff)

    def last_round_same_sum(p):  # r(0) + r(1) kept: only the final evaluation moves
        rp = _pad3(p["sumcheck"][2][-1])
        rp[1], rp[2] = (rp[1] + 1) % R, (rp[2] - 1) % R
        p["sumcheck"][2][-1] = rp
    add("last round, sum kept", FINAL, last_round_same_sum)

    def fourth(p):
        p["sumcheck"][2][0] = _pad3(p["sumcheck"][2][0]) + [1]
    add("fourth coefficient", SHAPE, fourth)

    def dropped(p):
        p["sumcheck"][2].pop()
    add("dropped round", SHAPE, dropped)

    def extra_eval(p):
        p["evaluations"].append(0)
    add("extra evaluation", SHAPE, extra_eval)

    def point(p):
        p["opening"][0][0] = (p["opening"][0][0] + 1) % R
    add("opening point", FINAL, point)

    def evaluation(p):
        p["opening"][1] = (p["opening"][1] + 1) % R
    add("opening evaluation", FINAL, evaluation)

    for a in range(4):
        def kzg_y(p, a=a):
            x, y, pi = p["opening"][3][a]
            p["opening"][3][a] = (x, (y + 1) % R, pi)
        add(f"KZG opening {mo.OPENINGS[a]}", OPENING, kzg_y)

    swapped = list(comms)
    if len(swapped) > 1:
        swapped[0], swapped[1] = swapped[1], swapped[0]
    else:
        swapped[0] = o.g1_add(swapped[0], o.G1_GEN)
    add("swapped commitment", OPENING, comms_=swapped)

    moved = [(j, list(z)) for j, z in claims]
    moved[-1][1][0] = (moved[-1][1][0] + 1) % R
    # the point moves t and with it s = sum t^i y_i.  A single claim has s = y_0
    # whatever t is: the transcript still differs, so round 1's message no
    # longer sums to round 0's value at the new challenge; with one round only
    # the combiner c_0 = eq(r, z_0) is left to fail
    single = ROUND if len(claims[0][1]) > 1 else FINAL
    add("changed claim point", SUM if len(claims) > 1 else single, claims_=moved)
    return out


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("n,P,k", CASES)
def test_restatement_accepts_its_proofs(n, P, k):
    polys, claims, kzg, comms, proof, state = _case(n, P, k)
    assert proof["evaluations"] == [o.mle_evaluate(polys[j], z) for j, z in claims]
    if k >= 2:
        assert claims[0][1] == claims[1][1]
    if k >= 3:
        assert set(claims[2][1]) <= {0, 1}
    vt = o.Transcript(DOMAIN)
    assert mo.verify(proof, comms, claims, kzg, vt) is None
    assert vt.state == state


@pytest.mark.parametrize("n,P,k", CASES)
def test_restatement_rejects_every_tamper(n, P, k):
    _, claims, kzg, comms, proof, _ = _case(n, P, k)
    for name, bad, cm, cl, msg in tampers(proof, comms, claims):
        with pytest.raises(ValueError) as e:
            mo.verify(bad, cm, cl, kzg, o.Transcript(DOMAIN))
        assert str(e.value) == msg, name


# ---------------------------------------------------------------- the product's verifier
@pytest.mark.parametrize("n,P,k", CASES)
def test_product_verifier_accepts_restated_proofs(n, P, k):
    q = _q()
    _, claims, _, comms, proof, state = _case(n, P, k)
    vk = q.KZG.verifier(tau=TAU)
    t = q.Transcript(DOMAIN)
    assert mo.to_product(q, proof).verify(comms, claims, vk, t) is None
    assert t.state == state
    # a deferring view collects the opening's four KZG claims and accepts too
    view = vk.deferring()
    t = q.Transcript(DOMAIN)
    mo.to_product(q, proof).verify(comms, claims, view, t)
    assert t.state == state and len(view.claims) == 4
    view.check()


@pytest.mark.parametrize("n,P,k", CASES)
def test_product_verifier_rejects_every_tamper(n, P, k):
    q = _q()
    _, claims, _, comms, proof, _ = _case(n, P, k)
    vk = q.KZG.verifier(tau=TAU)
    for name, bad, cm, cl, msg in tampers(proof, comms, claims):
        with pytest.raises(ValueError) as e:
            mo.to_product(q, bad).verify(cm, cl, vk, q.Transcript(DOMAIN))
        assert str(e.value) == msg, name


def test_product_verifier_defers_a_false_opening_to_the_batch():
    q = _q()
    _, claims, _, comms, proof, _ = _case(2, 3, 5)
    bad = copy.deepcopy(proof)
    x, y, pi = bad["opening"][3][2]
    bad["opening"][3][2] = (x, y, o.g1_add(pi, o.G1_GEN))  # y kept: the ML equation holds
    view = q.KZG.verifier(tau=TAU).deferring()
    p = mo.to_product(q, bad)
    view.labels[id(p.opening)] = "the batch opening"
    view.messages[id(p.opening)] = OPENING
    p.verify(comms, claims, view, q.Transcript(DOMAIN))
    with pytest.raises(ValueError, match=OPENING + r" \(the batch opening, s_opening"):
        view.check()


# ---------------------------------------------------------------- qg_g1_lincomb
def test_g1_lincomb_matches_naive_msm():
    q = _q()
    rnd = random.Random(5)
    G = o.G1_GEN
    pts = [o.g1_mul(G, rnd.randrange(R)) for _ in range(5)]
    sc = [rnd.randrange(R) for _ in range(5)]
    assert q.g1_lincomb(pts, sc) == o.g1_msm_naive(pts, sc)
    # an identity input, a zero scalar, a scalar of r - 1, a repeated point
    pts2, sc2 = [None, pts[0], pts[1], pts[1], pts[2]], [sc[0], 0, R - 1, 2, sc[3]]
    assert q.g1_lincomb(pts2, sc2) == o.g1_msm_naive(pts2, sc2)
    assert q.g1_lincomb([pts[0]], [1]) == pts[0]
    # identity results
    assert q.g1_lincomb([pts[0], pts[0]], [1, R - 1]) is None
    assert q.g1_lincomb([None], [7]) is None
    assert q.g1_lincomb([pts[0]], [0]) is None


def test_g1_lincomb_statuses():
    from quill_amd._lib import lib
    L = lib()
    xy, inf, s = (C.c_uint64 * 8)(), (C.c_uint8 * 1)(1), (C.c_uint64 * 4)()
    out, oinf = (C.c_uint64 * 8)(), C.c_uint8()
    assert L.qg_g1_lincomb(xy, inf, s, 1, out, C.byref(oinf)) == 0 and oinf.value == 1
    assert L.qg_g1_lincomb(None, inf, s, 1, out, C.byref(oinf)) == -1
    assert L.qg_g1_lincomb(xy, None, s, 1, out, C.byref(oinf)) == -1
    assert L.qg_g1_lincomb(xy, inf, None, 1, out, C.byref(oinf)) == -1
    assert L.qg_g1_lincomb(xy, inf, s, 1, None, C.byref(oinf)) == -1
    assert L.qg_g1_lincomb(xy, inf, s, 1, out, None) == -1
    assert L.qg_g1_lincomb(xy, inf, s, 0, out, C.byref(oinf)) == -1
    from quill_amd.field import g1_to_abi
    off, _ = g1_to_abi((1, 3))  # 9 != 1 + 3
    inf[0] = 0
    assert L.qg_g1_lincomb(off, inf, s, 1, out, C.byref(oinf)) == -1


# ---------------------------------------------------------------- wire format
@pytest.mark.parametrize("n,P,k", [(1, 1, 1), (2, 1, 3), (4, 3, 5)])
def test_multiopen_serialize_roundtrip(n, P, k):
    q = _q()
    _, _, _, _, proof, _ = _case(n, P, k)
    p = mo.to_product(q, proof)
    blob = q.serialize(p)
    # evaluations as Vec<Fr>, then SumcheckProof, then MLEvalProof
    head = o.ser_u64(k) + b"".join(o.ser_fr(y) for y in proof["evaluations"])
    assert blob[:len(head)] == head
    assert blob[len(head):] == q.serialize(p.sumcheck) + q.serialize(p.opening)
    back = q.deserialize(q.MultiOpenProof, blob)
    assert back == p and q.serialize(back) == blob
    for cut in (0, 7, len(head) - 1, len(head) + 9, len(blob) - 1):
        with pytest.raises(ValueError):
            q.deserialize(q.MultiOpenProof, blob[:cut])
    with pytest.raises(ValueError):
        q.deserialize(q.MultiOpenProof, blob + b"\0")


def test_abi_declares_the_entries():
    import os
    import re
    from quill_amd._lib import PROTOTYPES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "quill_gpu.h")) as fh:
        hdr = fh.read()
    for sym in ("qg_eq_multi_dev", "qg_mle_eval_multi_dev", "qg_lincomb_dev", "qg_g1_lincomb"):
        assert sym in PROTOTYPES
        assert re.search(r"\bint %s\(" % sym, hdr)


def test_trace_proof_flag_byte_round_trip():
    """a TraceProof with multi_openings: one flag byte after the two PIOP
    proofs, then the batches; the default layout is untouched"""
    q = _q()
    _, _, _, _, proof, _ = _case(2, 3, 5)
    m = mo.to_product(q, proof)
    sc = q.SumcheckProof(2, 0, [[1, 2], [3]])
    me = q.MultisetEqualityProof(o.G1_GEN, None, sc, m.opening, m.opening)
    head = (q.ZeroCheckProof(2, sc), q.PermutationCheckProof(me))
    default = q.TraceProof(*head, [m.opening] * 4, [m.opening], m.opening, m.opening, m.opening)
    prefix = q.serialize(head[0]) + q.serialize(head[1])
    blob = q.serialize(default)
    assert blob[:len(prefix) + 8] == prefix + o.ser_u64(4)
    assert q.deserialize(q.TraceProof, blob) == default
    for groups, flag in (([m, m], 0xFF), ([m], 0xFE)):
        tp = q.TraceProof(*head, [], [], None, None, None, groups)
        blob = q.serialize(tp)
        assert blob == prefix + bytes([flag]) + q.serialize(m) * len(groups)
        assert q.deserialize(q.TraceProof, blob) == tp
        hp = q.HyperPlonkProof([o.G1_GEN], [tp, default])
        assert q.deserialize(q.HyperPlonkProof, q.serialize(hp)) == hp
        with pytest.raises(ValueError):
            q.deserialize(q.TraceProof, blob[:-1])
        with pytest.raises(ValueError):
            q.deserialize(q.TraceProof, blob + b"\0")
