"""LookupProof.verify / SetInclusionProof.verify (host mirrors of lookup.rs:87-141
and set_inclusion.rs:237-347) on the CPU: the oracle proves the XOR-42 byte
lookup (lookup.rs:197-297) at 2^5 source rows against the 2^8-row table, the
proof is converted to the quill_amd dataclasses, and the product verifier

  * accepts it and ends in the oracle verifier's transcript state;
  * raises the reference's error string for one tamper per string, and the
    same string as the oracle verifier does for the same tamper;
  * rejects a proof for a source column with one wrong row (proved by the
    oracle with the honest multiplicities)."""
import random

import pytest

import pairing_oracle as po
import quill_oracle as o

R = o.R_MOD
TAU = 0x1234567890ABCDEF1122334455667788
NS, ND = 5, 8
DOMAIN = b"lookup_verify"


def _q():
    import quill_amd
    return quill_amd


def _mle_from_oracle(p):
    q = _q()
    return q.MLEvalProof(list(p.evaluation_point), p.evaluation, p.s_comm,
                         *[q.KZGOpeningProof(*t) for t in (p.poly_opening, p.poly_opening_inv,
                                                          p.s_opening, p.s_opening_inv)])


def _sc_from_oracle(s):
    return _q().SumcheckProof(s.num_vars, s.claimed_sum % R, [list(p) for p in s.r_polys])


def _to_product(op):
    """oracle SetInclusionProof -> quill_amd.LookupProof (same values)"""
    q = _q()
    return q.LookupProof(q.SetInclusionProof(
        op.denom_left_commitment, op.denom_right_commitment,
        _sc_from_oracle(op.sumcheck_proof_left), _sc_from_oracle(op.sumcheck_proof_right),
        _mle_from_oracle(op.opening_proof_denom_left),
        _mle_from_oracle(op.opening_proof_denom_right)))


def _to_oracle(proof):
    """quill_amd.LookupProof -> oracle SetInclusionProof (same values)"""
    def opening(p):
        return o.MLEvalProof(list(p.evaluation_point), p.evaluation, p.s_comm,
                             *[(getattr(p, k).x, getattr(p, k).y, getattr(p, k).proof)
                               for k in ("poly_opening", "poly_opening_inv", "s_opening",
                                         "s_opening_inv")])
    sp = proof.set_inclusion_proof
    return o.SetInclusionProof(
        sp.denom_left_commitment, sp.denom_right_commitment,
        o.SumcheckProof(sp.sumcheck_proof_left.num_vars, sp.sumcheck_proof_left.claimed_sum,
                        [list(p) for p in sp.sumcheck_proof_left.r_polys]),
        o.SumcheckProof(sp.sumcheck_proof_right.num_vars, sp.sumcheck_proof_right.claimed_sum,
                        [list(p) for p in sp.sumcheck_proof_right.r_polys]),
        opening(sp.opening_proof_denom_left), opening(sp.opening_proof_denom_right))


class _Case:
    """one oracle proof of the XOR-42 lookup and the claims a verifier is given"""

    def __init__(self, okzg, wrong_row=None, shift_opening=None):
        rnd = random.Random(42)
        c1, c2 = list(range(256)), [i ^ 42 for i in range(256)]
        by = [rnd.randrange(256) for _ in range(1 << NS)]
        s1, s2 = list(by), [b ^ 42 for b in by]
        mult = [0] * 256
        for b in by:
            mult[b] += 1
        if wrong_row is not None:  # the honest m, one source row that breaks the relation
            s2[wrong_row] = (s2[wrong_row] + 1) % 256
        ss, ds = o.VirtualPolynomialStore(NS), o.VirtualPolynomialStore(ND)
        for tb in (s1, s2):
            ss.allocate_polynomial(tb)
        for tb in (c1, c2, mult):
            ds.allocate_polynomial(tb)
        sc = [ss.new_virtual_from_input(0), ss.new_virtual_from_input(1)]
        dc = [ds.new_virtual_from_input(0), ds.new_virtual_from_input(1)]
        m = ds.new_virtual_from_input(2)
        real = o.MLEvalProof.prove
        calls = []

        def prove(poly, pt, kzg, t):
            # shift_opening = k: the k-th opening (0 left, 1 right) is a valid
            # opening, in the prover's own transcript, at another point
            if shift_opening == len(calls):
                pt = [(pt[0] + 1) % R] + list(pt[1:])
            calls.append(1)
            return real(poly, pt, kzg, t)
        o.MLEvalProof.prove = staticmethod(prove)
        try:
            self.oproof, (pl, pr) = o.lookup_prove(ss, sc, ds, dc, m, o.Transcript(DOMAIN), okzg)
        finally:
            o.MLEvalProof.prove = staticmethod(real)
        assert len(calls) == 2
        self.src = [(pl, o.mle_evaluate(s1, pl)), (pl, o.mle_evaluate(s2, pl))]
        self.dst = [(pr, o.mle_evaluate(c1, pr)), (pr, o.mle_evaluate(c2, pr))]
        self.m = (pr, o.mle_evaluate(mult, pr))

    def claims(self):
        E = _q().EvaluationClaim
        return ([E(list(p), e) for p, e in self.src], [E(list(p), e) for p, e in self.dst],
                E(list(self.m[0]), self.m[1]))


@pytest.fixture(scope="module")
def okzg():
    return o.KZG(1 << ND, TAU)


@pytest.fixture(scope="module")
def honest(okzg):
    return _Case(okzg)


def _verify_both(proof, src, dst, m, okzg):
    """(product error or None, oracle error or None, product state, oracle state)"""
    q = _q()
    t, ot = q.Transcript(DOMAIN), o.Transcript(DOMAIN)
    err = oerr = None
    try:
        proof.verify(t, q.KZG.verifier(tau=TAU), src, dst, m)
    except ValueError as e:
        err = str(e)
    try:
        o.lookup_verify(_to_oracle(proof), ot, okzg, [(c.point, c.evaluation) for c in src],
                        [(c.point, c.evaluation) for c in dst], (m.point, m.evaluation))
    except ValueError as e:
        oerr = str(e)
    return err, oerr, t.state, ot.state


def test_lookup_verify_accepts_oracle_proof(honest, okzg):
    proof = _to_product(honest.oproof)
    src, dst, m = honest.claims()
    err, oerr, st, ost = _verify_both(proof, src, dst, m, okzg)
    assert err is None and oerr is None
    assert st == ost


def test_set_inclusion_verify_direct(honest):
    """SetInclusionProof.verify on its own, fed the batched claims lookup.rs:114-129 forms"""
    q = _q()
    proof = _to_product(honest.oproof).set_inclusion_proof
    src, dst, m = honest.claims()
    t = q.Transcript(DOMAIN)
    t.append_u64(2)
    alpha = t.draw_field_element()
    se = (src[0].evaluation + alpha * src[1].evaluation) % R
    de = (dst[0].evaluation + alpha * dst[1].evaluation) % R
    proof.verify(t, q.KZG.verifier(tau=TAU), q.EvaluationClaim(src[0].point, se),
                 q.EvaluationClaim(dst[0].point, de), m)
    with pytest.raises(ValueError, match="Left sumcheck evaluation mismatch"):
        t = q.Transcript(DOMAIN)
        t.append_u64(2)
        t.draw_field_element()
        proof.verify(t, q.KZG.verifier(tau=TAU), q.EvaluationClaim(src[0].point, (se + 1) % R),
                     q.EvaluationClaim(dst[0].point, de), m)


def _bump_point(c):
    c.point[0] = (c.point[0] + 1) % R


TAMPERS = [
    # a changed commitment changes every later challenge: the left sumcheck's
    # second round no longer chains (the reference fails there too)
    ("comm_left", "Sumcheck polynomial does not sum to previous value"),
    ("comm_right", "Sumcheck polynomial does not sum to previous value"),
    ("sum_left", "Sumcheck polynomial does not sum to previous value"),
    ("sum_right", "Sumcheck polynomial does not sum to previous value"),
    ("open_left_eval", "Left denominator opening proof failed"),
    ("open_right_eval", "Right denominator opening proof failed"),
    ("src_points", "Mismatched evaluation points for set inclusion"),
    ("dst_points", "Mismatched evaluation points for set inclusion"),
    ("m_point", "Mismatched evaluation points for set inclusion"),
    ("src_point_one", "Lookup evaluation points for columns are inconsistent"),
    ("src_eval", "Left sumcheck evaluation mismatch"),
    ("dst_eval", "Right sumcheck evaluation mismatch"),
    ("m_eval", "Right sumcheck evaluation mismatch"),
    ("dest_claims_short", "Mismatched lookup evaluation vector lengths"),
]


@pytest.mark.parametrize("where,msg", TAMPERS)
def test_lookup_verify_rejects_tampering(honest, okzg, where, msg):
    proof = _to_product(honest.oproof)
    sp = proof.set_inclusion_proof
    src, dst, m = honest.claims()
    if where == "comm_left":
        sp.denom_left_commitment = po.g1_add(sp.denom_left_commitment, po.G1_GEN)
    elif where == "comm_right":
        sp.denom_right_commitment = po.g1_add(sp.denom_right_commitment, po.G1_GEN)
    elif where == "sum_left":
        sp.sumcheck_proof_left.claimed_sum = (sp.sumcheck_proof_left.claimed_sum + 1) % R
    elif where == "sum_right":
        sp.sumcheck_proof_right.claimed_sum = (sp.sumcheck_proof_right.claimed_sum + 1) % R
    elif where == "open_left_eval":
        sp.opening_proof_denom_left.evaluation = (sp.opening_proof_denom_left.evaluation + 1) % R
    elif where == "open_right_eval":
        sp.opening_proof_denom_right.evaluation = (sp.opening_proof_denom_right.evaluation + 1) % R
    elif where == "src_points":
        for c in src:
            _bump_point(c)
    elif where == "dst_points":
        for c in dst:
            _bump_point(c)
    elif where == "m_point":
        _bump_point(m)
    elif where == "src_point_one":
        _bump_point(src[1])
    elif where == "src_eval":
        src[1].evaluation = (src[1].evaluation + 1) % R
    elif where == "dst_eval":
        dst[0].evaluation = (dst[0].evaluation + 1) % R
    elif where == "m_eval":
        m.evaluation = (m.evaluation + 1) % R
    elif where == "dest_claims_short":
        dst = dst[:1]
    else:
        raise AssertionError(where)
    err, oerr, _, _ = _verify_both(proof, src, dst, m, okzg)
    assert err == msg
    assert oerr == msg


@pytest.mark.parametrize("which,msg", [
    (0, "Left sumcheck point does not match PCS opening point"),
    (1, "Right sumcheck point does not match PCS opening point"),
])
def test_lookup_verify_rejects_opening_at_another_point(okzg, which, msg):
    """the opening is valid (made by the prover in its own transcript), but at a
    point that is not the sumcheck's"""
    case = _Case(okzg, shift_opening=which)
    proof = _to_product(case.oproof)
    src, dst, m = case.claims()
    sp = proof.set_inclusion_proof
    opening = sp.opening_proof_denom_left if which == 0 else sp.opening_proof_denom_right
    assert opening.point() != (src if which == 0 else dst)[0].point
    err, oerr, _, _ = _verify_both(proof, src, dst, m, okzg)
    assert err == msg
    assert oerr == msg


def test_lookup_verify_rejects_wrong_source_row(okzg):
    """one source row (b, b ^ 42 + 1) that is in no table row, proved with the
    honest m: every sumcheck and opening is consistent, the two log-derivative
    sums differ"""
    case = _Case(okzg, wrong_row=7)
    proof = _to_product(case.oproof)
    src, dst, m = case.claims()
    err, oerr, _, _ = _verify_both(proof, src, dst, m, okzg)
    assert err == "Log-derivative sums do not match"
    assert oerr == "Log-derivative sums do not match"
