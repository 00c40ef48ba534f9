"""HyperPlonk.prove(multi_open=True): each trace's openings as two multi-point
batch openings, on the circuits tests/test_gpu_hyperplonk.py proves (8 and 64
rows, one and two traces) and the 16-column circuit at 8 rows.

  * the proof verifies sequentially and batched (host fold and device fold)
    and the verifier ends in the prover's transcript state;
  * the transcript up to trace 0's openings is the default one, so the
    evaluations in trace 0's batches equal those of the default proof's openings;
  * the default proof is byte-identical with the argument left out;
  * a tampered evaluation or KZG opening in either batch of either trace is
    rejected, under batch=True with the batch's label;
  * the proof survives the wire, and holds 4 ML openings per trace."""
import dataclasses

import pytest

import pairing_oracle as po
import quill_oracle as o

pytestmark = pytest.mark.gpu
R = o.R_MOD
TAU = 0x48595045524C4F4E4B
CONFIGS = ["fib8", "fibmod8", "modfib64", "wide8"]
_CACHE = {}


def _q():
    import quill_amd
    return quill_amd


def _setup(dev, name):
    """(pcs, hp, vk, default proof, multi-open proof, its prover's final state),
    proven once per configuration"""
    if name not in _CACHE:
        q = _q()
        if name == "wide8":
            from test_gpu_generic import _wide_circuit_device, _wide_witness
            pcs = q.KZG.trusted_setup(16 * 8, TAU, dev)
            hp = q.HyperPlonk.preprocess([_wide_circuit_device(8)], pcs)
            ws = [_wide_witness(8)]
        else:
            from test_gpu_hyperplonk import _device_setup
            rows, which = {"fib8": (8, ("fib",)), "fibmod8": (8, ("fib", "mod")),
                           "modfib64": (64, ("mod", "fib"))}[name]
            pcs, hp, ws = _device_setup(dev, rows, which)
        default = hp.prove(pcs, ws)
        explicit = hp.prove(pcs, ws, multi_open=False)
        assert q.serialize(default) == q.serialize(explicit)
        multi = hp.prove(pcs, ws, multi_open=True)
        _CACHE[name] = (pcs, hp, hp.to_vk(), default, multi, hp.last_transcript.state)
    return _CACHE[name]


def _ml_openings(obj) -> int:
    """MLEvalProofs reachable from a proof object"""
    q = _q()
    if isinstance(obj, q.MLEvalProof):
        return 1
    if isinstance(obj, (list, tuple)):
        return sum(_ml_openings(x) for x in obj)
    if dataclasses.is_dataclass(obj):
        return sum(_ml_openings(getattr(obj, f.name)) for f in dataclasses.fields(obj))
    return 0


@pytest.mark.parametrize("name", CONFIGS)
def test_multi_open_proof_verifies(dev, name):
    pcs, hp, vk, default, multi, final = _setup(dev, name)
    assert multi.verify(vk, pcs).state == final
    assert multi.verify(vk, pcs, batch=True).state == final
    assert multi.verify(vk, pcs, batch=True, dev=dev).state == final
    # the default proof still verifies, and the witness commitments are shared
    assert default.verify(vk, pcs).state != final
    assert multi.witness_commitment == default.witness_commitment


@pytest.mark.parametrize("name", CONFIGS)
def test_shape_and_opening_count(dev, name):
    _, hp, vk, default, multi, _ = _setup(dev, name)
    for tp, tvk in zip(multi.trace_proofs, vk):
        npub = len(tvk.public_columns_commitments)
        assert npub > 0 and len(tp.multi_openings) == 2
        assert (tp.openings_zero_check, tp.openings_public) == ([], [])
        assert tp.opening_id is None and tp.opening_permutation is None
        assert tp.opening_permutation_trace is None
        assert len(tp.multi_openings[0].evaluations) == tvk.circuit.num_cols() + 3
        assert len(tp.multi_openings[1].evaluations) == npub
    traces = len(multi.trace_proofs)
    assert _ml_openings(multi) == 4 * traces  # 2 Logup denominators + 2 batches per trace
    assert _ml_openings(default) == sum(2 + tvk.circuit.num_cols()
                                        + len(tvk.public_columns_commitments) + 3 for tvk in vk)
    assert all(tp.multi_openings is None for tp in default.trace_proofs)


@pytest.mark.parametrize("name", CONFIGS)
def test_trace0_evaluations_equal_the_default_openings(dev, name):
    _, _, _, default, multi, _ = _setup(dev, name)
    d, m = default.trace_proofs[0], multi.trace_proofs[0]
    assert m.zero_check_proof == d.zero_check_proof
    assert m.permutation_check_proof == d.permutation_check_proof
    assert m.multi_openings[0].evaluations == (
        [op.evaluation for op in d.openings_zero_check]
        + [d.opening_id.evaluation, d.opening_permutation.evaluation,
           d.opening_permutation_trace.evaluation])
    assert m.multi_openings[1].evaluations == [op.evaluation for op in d.openings_public]


@pytest.mark.parametrize("name", CONFIGS)
def test_wire_round_trip(dev, name):
    q = _q()
    pcs, _, vk, default, multi, final = _setup(dev, name)
    blob = q.serialize(multi)
    back = q.deserialize(q.HyperPlonkProof, blob)
    assert back == multi and q.serialize(back) == blob
    assert back.verify(vk, pcs).state == final
    assert len(blob) < len(q.serialize(default))
    assert q.deserialize(q.HyperPlonkProof, q.serialize(default)) == default
    for cut in (len(blob) - 1, len(blob) // 2):
        with pytest.raises(ValueError):
            q.deserialize(q.HyperPlonkProof, blob[:cut])


GROUPS = ("witness/id/permutation", "public-column")


@pytest.mark.parametrize("name", ["fibmod8", "modfib64"])
@pytest.mark.parametrize("trace", [0, 1])
@pytest.mark.parametrize("group", [0, 1])
def test_tampering_is_rejected(dev, name, trace, group):
    q = _q()
    pcs, _, vk, _, multi, _ = _setup(dev, name)
    blob = q.serialize(multi)

    def fresh():
        p = q.deserialize(q.HyperPlonkProof, blob)
        return p, p.trace_proofs[trace].multi_openings[group]

    p, m = fresh()
    m.evaluations[-1] = (m.evaluations[-1] + 1) % R
    for kw in ({}, {"batch": True}, {"batch": True, "dev": dev}):
        with pytest.raises(ValueError):
            p.verify(vk, pcs, **kw)
    p, m = fresh()
    m.opening.s_opening_inv.proof = po.g1_add(m.opening.s_opening_inv.proof, po.G1_GEN)
    with pytest.raises(ValueError, match="^Multi-open opening verification failed$"):
        p.verify(vk, pcs)
    label = (rf"Multi-open opening verification failed \(trace {trace} {GROUPS[group]} "
             r"multi-open opening, s_opening_inv; batched claim")
    with pytest.raises(ValueError, match=label):
        p.verify(vk, pcs, batch=True)
    with pytest.raises(ValueError, match=label):
        p.verify(vk, pcs, batch=True, dev=dev)
    # a batch moved to the other trace, and the two batches of a trace swapped
    p, _ = fresh()
    a, b = p.trace_proofs
    a.multi_openings, b.multi_openings = b.multi_openings, a.multi_openings
    with pytest.raises(ValueError):
        p.verify(vk, pcs)
    p, _ = fresh()
    p.trace_proofs[trace].multi_openings.reverse()
    with pytest.raises(ValueError):
        p.verify(vk, pcs)


def test_multi_open_on_a_sharded_device_raises(dev):
    q = _q()
    _, hp, _, _, _, _ = _setup(dev, "fib8")
    group = q.Device.loopback_group(2)
    d = q.Device(0)
    d.attach_loopback(group, 0)
    with pytest.raises(ValueError, match="sharded"):
        hp.prove(q.KZG(d, None, 64, TAU), [], multi_open=True)
    d.close()
    q.lib().qg_loopback_destroy(group)
