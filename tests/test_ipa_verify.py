"""InnerProductProof on the CPU (no GPU needed: qg_ipa_verify, the pairing and
the transcript are host code in libquill_gpu.so).

  * the restatement of ipa.rs prove / verify (tests/ipa_restatement.py) passes
    the reference's own KATs (ipa.rs:230, :273), accepts its own proofs and
    rejects a tampered inner product;
  * qg_ipa_verify (ipa.rs:160-202) accepts the restated prover's proofs, ends in
    the restated verifier's transcript state, and rejects every tampered field,
    leaving the transcript untouched when a KZG check fails;
  * serialize -> deserialize is the identity for InnerProductProof; truncated
    input raises;
  * the header and the ctypes table agree on the new struct."""
import ctypes as C
import random
import re

import pytest

import ipa_restatement as ipa
import pairing_oracle as po
import quill_oracle as o

R = o.R_MOD
TAU = 0x48595045524C4F4E4B
DOMAIN = b"ipa_verify"


def _q():
    import quill_amd
    return quill_amd


def _case(nf, ng, seed=None):
    rnd = random.Random(nf * 1000 + ng if seed is None else seed)
    f = [rnd.randrange(R) for _ in range(nf)]
    g = [rnd.randrange(R) for _ in range(ng)]
    kzg = o.KZG(max(nf, ng, 2), TAU, points=[])
    ot = o.Transcript(DOMAIN)
    proof = ipa.prove(f, g, kzg, ot)
    return f, g, kzg, proof, ot


# ---------------------------------------------------------------- the restatement itself
def test_restatement_kats():
    kzg = o.KZG(8, TAU, points=[])
    p = ipa.prove([1, 2, 3], [4, 5, 6], kzg, o.Transcript(DOMAIN))   # ipa.rs:230
    assert p[0] == 32
    p = ipa.prove([1, 2, 3], [4, 5], kzg, o.Transcript(DOMAIN))      # ipa.rs:273
    assert p[0] == 14
    assert ipa.prove([1, 2], [4, 5, 6], kzg, o.Transcript(DOMAIN))[0] == 14
    # no S at all, and an all-zero S: identity commitment
    for f, g in (([7], [9]), ([1, 2, 3], [])):
        p = ipa.prove(f, g, kzg, o.Transcript(DOMAIN))
        assert p[1] is None and p[6] == (p[6][0], 0, None)


@pytest.mark.parametrize("nf,ng", [(3, 3), (3, 2), (1, 1), (17, 9)])
def test_restatement_accepts_its_proof_and_rejects_tampering(nf, ng):
    f, g, kzg, proof, ot = _case(nf, ng)
    c1, c2 = kzg.commit(f), kzg.commit(g)
    vt = o.Transcript(DOMAIN)
    assert ipa.verify(proof, c1, c2, kzg, vt)
    assert vt.state == ot.state
    bad = ((proof[0] + 1) % R,) + proof[1:]
    assert not ipa.verify(bad, c1, c2, kzg, o.Transcript(DOMAIN))


# ---------------------------------------------------------------- qg_ipa_verify
@pytest.mark.parametrize("nf,ng", [(3, 3), (3, 2), (1, 1), (17, 9)])
def test_ipa_verify_restated_proofs(nf, ng):
    q = _q()
    f, g, kzg, oproof, ot = _case(nf, ng)
    vk = q.KZG.verifier(tau=TAU)
    c1, c2 = kzg.commit(f), kzg.commit(g)
    proof = ipa.to_product(q, oproof)
    t = q.Transcript(DOMAIN)
    assert proof.verify(c1, c2, vk, t)
    vt = o.Transcript(DOMAIN)
    assert ipa.verify(oproof, c1, c2, kzg, vt)
    assert t.state == vt.state == ot.state
    fresh = q.Transcript(DOMAIN).state

    def rejected(bad, a=c1, b=c2, untouched=True):
        t = q.Transcript(DOMAIN)
        assert not bad.verify(a, b, vk, t)
        assert (t.state == fresh) == untouched

    # the inner product enters no KZG check: the equation fails, after the appends
    bad = ipa.to_product(q, oproof)
    bad.inner_product = (bad.inner_product + 1) % R
    rejected(bad, untouched=False)
    # each of the six y, the S commitment, each commitment: a KZG check fails first
    for name in ipa.OPENINGS:
        bad = ipa.to_product(q, oproof)
        op = getattr(bad, name)
        op.y = (op.y + 1) % R
        rejected(bad)
    bad = ipa.to_product(q, oproof)
    bad.s_comm = po.g1_add(bad.s_comm, po.G1_GEN)
    rejected(bad)
    rejected(proof, a=po.g1_add(c1, po.G1_GEN))
    rejected(proof, b=po.g1_add(c2, po.G1_GEN))


def test_ipa_verify_statuses():
    q = _q()
    from quill_amd._lib import IpaProof, lib
    f, g, kzg, oproof, _ = _case(3, 3)
    vk = q.KZG.verifier(tau=TAU)._vk()
    xy = (C.c_uint64 * 8)()
    st = (C.c_uint8 * 32)()
    ok = C.c_int()
    pr = IpaProof()
    L = lib()
    assert L.qg_ipa_verify(None, xy, 1, xy, 1, C.byref(pr), st, C.byref(ok)) == -1
    assert L.qg_ipa_verify(C.byref(vk), None, 1, xy, 1, C.byref(pr), st, C.byref(ok)) == -1
    assert L.qg_ipa_verify(C.byref(vk), xy, 1, None, 1, C.byref(pr), st, C.byref(ok)) == -1
    assert L.qg_ipa_verify(C.byref(vk), xy, 1, xy, 1, None, st, C.byref(ok)) == -1
    assert L.qg_ipa_verify(C.byref(vk), xy, 1, xy, 1, C.byref(pr), None, C.byref(ok)) == -1
    assert L.qg_ipa_verify(C.byref(vk), xy, 1, xy, 1, C.byref(pr), st, None) == -1


# ---------------------------------------------------------------- wire format
@pytest.mark.parametrize("nf,ng", [(3, 2), (1, 1), (17, 9)])
def test_ipa_serialize_roundtrip(nf, ng):
    q = _q()
    _, _, _, oproof, _ = _case(nf, ng)
    proof = ipa.to_product(q, oproof)
    blob = q.serialize(proof)
    # inner_product, s_comm, six (x, y, proof): struct order, nothing else
    assert len(blob) == 32 + 64 + 6 * (32 + 32 + 64)
    assert blob[:32] == o.ser_fr(oproof[0]) and blob[32:96] == o.ser_g1(oproof[1])
    assert blob[96:96 + 128] == (o.ser_fr(oproof[2][0]) + o.ser_fr(oproof[2][1])
                                 + o.ser_g1(oproof[2][2]))
    back = q.deserialize(q.InnerProductProof, blob)
    assert back == proof
    assert q.serialize(back) == blob
    for cut in (0, 31, 95, 96 + 127, len(blob) - 1):
        with pytest.raises(ValueError):
            q.deserialize(q.InnerProductProof, blob[:cut])
    with pytest.raises(ValueError):
        q.deserialize(q.InnerProductProof, blob + b"\0")
    with pytest.raises(ValueError):  # a non-canonical inner product
        q.deserialize(q.InnerProductProof, R.to_bytes(32, "little") + blob[32:])


# ---------------------------------------------------------------- ABI
def test_ipa_struct_layout_matches_header():
    """qg_ipa_proof: the reference's field order (ipa.rs:40-53), padded like
    qg_mle_proof, and the same layout in the ctypes mirror"""
    import os
    from quill_amd._lib import PROTOTYPES, IpaProof, KzgOpening
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "quill_gpu.h")) as fh:
        hdr = fh.read()
    body = re.search(r"typedef struct qg_ipa_proof \{(.*?)\} qg_ipa_proof;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?;", body)
    assert names == ["inner_product", "s_comm_xy", "s_comm_inf", "_pad", *ipa.OPENINGS]
    assert [n for n, _ in IpaProof._fields_] == names
    assert C.sizeof(IpaProof) == 32 + 64 + 8 + 6 * C.sizeof(KzgOpening)
    assert IpaProof.f_opening.offset == 104
    for sym in ("qg_ipa_prove", "qg_ipa_prove_dev", "qg_ipa_verify"):
        assert sym in PROTOTYPES
        assert re.search(r"\bint %s\(" % sym, hdr)
