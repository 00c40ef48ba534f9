"""HyperPlonk.prove(pcs.folding(), ...): every ML opening of the proof folded,
with and without multi_open=True, on the circuits
tests/test_gpu_hyperplonk_multiopen.py proves.

  * the proof verifies sequentially, batched on the host and batched with the
    device fold, and the verifier ends in the prover's transcript state;
  * it survives serialize -> deserialize(..., opening=FoldedMLEvalProof) -> verify;
  * a tampered y or w is rejected;
  * a default proof of the same inputs is byte-identical to one made before any
    folded call in the process."""
import dataclasses

import pytest

import pairing_oracle as po
import quill_oracle as o

pytestmark = pytest.mark.gpu
R = o.R_MOD
CONFIGS = ["fib8", "fibmod8", "modfib64"]
_CACHE = {}


def _q():
    import quill_amd
    return quill_amd


def _setup(dev, name):
    """per configuration, proven once: the default proof's bytes BEFORE any
    folded call, then folded proofs (plain and multi-open) with their provers'
    final states, then the default proof's bytes again"""
    if name not in _CACHE:
        q = _q()
        from test_gpu_hyperplonk import _device_setup
        rows, which = {"fib8": (8, ("fib",)), "fibmod8": (8, ("fib", "mod")),
                       "modfib64": (64, ("mod", "fib"))}[name]
        pcs, hp, ws = _device_setup(dev, rows, which)
        before = q.serialize(hp.prove(pcs, ws))
        folded = {}
        for multi in (False, True):
            p = hp.prove(pcs.folding(), ws, multi_open=multi)
            folded[multi] = (p, hp.last_transcript.state)
        after = q.serialize(hp.prove(pcs, ws))
        _CACHE[name] = (pcs, hp.to_vk(), folded, before, after)
    return _CACHE[name]


def _openings(obj, cls) -> list:
    """the instances of cls reachable from a proof object"""
    if isinstance(obj, cls):
        return [obj]
    if isinstance(obj, (list, tuple)):
        return [x for y in obj for x in _openings(y, cls)]
    if dataclasses.is_dataclass(obj):
        return [x for f in dataclasses.fields(obj) for x in _openings(getattr(obj, f.name), cls)]
    return []


@pytest.mark.parametrize("multi", [False, True], ids=["plain", "multi_open"])
@pytest.mark.parametrize("name", CONFIGS)
def test_folded_proof_verifies(dev, name, multi):
    q = _q()
    pcs, vk, folded, _, _ = _setup(dev, name)
    proof, final = folded[multi]
    assert proof.verify(vk, pcs).state == final
    assert proof.verify(vk, pcs, batch=True).state == final
    assert proof.verify(vk, pcs, batch=True, dev=dev).state == final
    # every ML opening of the proof is folded
    assert _openings(proof, q.MLEvalProof) == []
    n = len(_openings(proof, q.FoldedMLEvalProof))
    if multi:
        assert n == 4 * len(proof.trace_proofs)
    else:
        assert n == sum(2 + t.circuit.num_cols() + len(t.public_columns_commitments) + 3
                        for t in vk)


@pytest.mark.parametrize("multi", [False, True], ids=["plain", "multi_open"])
@pytest.mark.parametrize("name", CONFIGS)
def test_wire_round_trip(dev, name, multi):
    q = _q()
    pcs, vk, folded, before, _ = _setup(dev, name)
    proof, final = folded[multi]
    blob = q.serialize(proof)
    back = q.deserialize(q.HyperPlonkProof, blob, opening=q.FoldedMLEvalProof)
    assert back == proof and q.serialize(back) == blob
    assert back.verify(vk, pcs).state == final
    # 256 bytes less per opening than the same proof with plain openings
    if not multi:
        assert len(blob) == len(before) - 256 * len(_openings(proof, q.FoldedMLEvalProof))
    with pytest.raises(ValueError):
        q.deserialize(q.HyperPlonkProof, blob)
    with pytest.raises(ValueError):
        q.deserialize(q.HyperPlonkProof, blob[:-1], opening=q.FoldedMLEvalProof)


@pytest.mark.parametrize("multi", [False, True], ids=["plain", "multi_open"])
@pytest.mark.parametrize("field", ["y_poly", "y_s_inv", "w", "w_inv"])
def test_tampering_is_rejected(dev, field, multi):
    q = _q()
    pcs, vk, folded, _, _ = _setup(dev, "fibmod8")
    blob = q.serialize(folded[multi][0])
    for which in (0, -1):  # the first and the last opening of the proof
        p = q.deserialize(q.HyperPlonkProof, blob, opening=q.FoldedMLEvalProof)
        op = _openings(p, q.FoldedMLEvalProof)[which]
        v = getattr(op, field)
        setattr(op, field, (v + 1) % R if field.startswith("y") else po.g1_add(v, po.G1_GEN))
        for kw in ({}, {"batch": True}, {"batch": True, "dev": dev}):
            with pytest.raises(ValueError):
                p.verify(vk, pcs, **kw)


@pytest.mark.parametrize("name", CONFIGS)
def test_default_proof_is_unchanged(dev, name):
    q = _q()
    pcs, vk, _, before, after = _setup(dev, name)
    assert before == after
    p = q.deserialize(q.HyperPlonkProof, before)
    assert _openings(p, q.FoldedMLEvalProof) == []
    p.verify(vk, pcs)
