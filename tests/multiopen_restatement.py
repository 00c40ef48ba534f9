"""The multi-point batch opening (HyperPlonk paper, section 3.8) restated on the
oracle's primitives alone, prover and verifier, for the tests of the device
prover and of the product's host verifier.  `kzg` is an
`o.KZG(max_degree, tau, points=[])`: it commits and opens through the trapdoor.

Statement: k claims f_{j_i}(z_i) = y_i over P polynomials of n variables.
  1. absorb n, P, k (u64); per claim j_i (u64), z_i (Fr vector), y_i (Fr)
  2. t = draw; w_i = t^i; s = sum_i w_i y_i
  3. g_j = sum_{i: j_i = j} w_i eq(., z_i); sumcheck of sum_j f_j g_j with
     claimed sum s -> (r, e)
  4. c_j = sum_{i: j_i = j} w_i eq(r, z_i); MLEvalProof of sum_j c_j f_j at r,
     whose evaluation is e; the verifier checks it against sum_j c_j C_j

A proof is plain data, so a test can copy and tamper with it:
    {"evaluations": [y_i],
     "sumcheck": [num_vars, claimed_sum, r_polys],
     "opening": [point, evaluation, s_comm, [(x, y, pi)] * 4]}
(the four KZG openings in MLEvalProof's field order)."""
import random

import quill_oracle as o

R = o.R_MOD
OPENINGS = ("poly_opening", "poly_opening_inv", "s_opening", "s_opening_inv")


def absorb_and_draw(n, P, claims, evaluations, t):
    t.append_u64(n)
    t.append_u64(P)
    t.append_u64(len(claims))
    for (j, z), y in zip(claims, evaluations):
        t.append_u64(j)
        t.append_fr_vec(list(z))
        t.append_fr(y)
    tt = t.draw_field_element()
    w = [pow(tt, i, R) for i in range(len(claims))]
    return w, sum(wi * y for wi, y in zip(w, evaluations)) % R


def combiners(P, claims, w, r):
    c = [0] * P
    for (j, z), wi in zip(claims, w):
        c[j] = (c[j] + wi * o.eq_eval(list(r), list(z))) % R
    return c


def prove(polys, claims, kzg, t):
    P, n = len(polys), len(claims[0][1])
    N = 1 << n
    assert all(len(f) == N for f in polys)
    assert {j for j, _ in claims} == set(range(P)), "every polynomial needs a claim"
    ys = [o.mle_evaluate(polys[j], z) for j, z in claims]
    w, s = absorb_and_draw(n, P, claims, ys, t)
    gs = [[0] * N for _ in range(P)]
    for (j, z), wi in zip(claims, w):
        for x, e in enumerate(o.fast_eq_eval_hypercube(n, z)):
            gs[j][x] = (gs[j][x] + wi * e) % R
    store = o.VirtualPolynomialStore(n)
    for f in polys:
        store.allocate_polynomial(f)
    for g in gs:
        store.allocate_polynomial(g)
    h = o.Expr.input(0) * o.Expr.input(P)
    for j in range(1, P):
        h = h + o.Expr.input(j) * o.Expr.input(P + j)
    sc, (r, e) = o.SumcheckProof.prove_fast(n, store, store.new_virtual_from_expr(h), s, t)
    c = combiners(P, claims, w, r)
    fstar = [sum(cj * f[x] for cj, f in zip(c, polys)) % R for x in range(N)]
    op = o.MLEvalProof.prove(fstar, r, kzg, t)
    assert op.evaluation == e, "multi-open final evaluation mismatch"
    return {"evaluations": ys,
            "sumcheck": [sc.num_vars, sc.claimed_sum, [list(rp) for rp in sc.r_polys]],
            "opening": [list(op.evaluation_point), op.evaluation, op.s_comm,
                        [tuple(getattr(op, name)) for name in OPENINGS]]}


def verify(proof, commitments, claims, kzg, t):
    """raises ValueError with the product's messages; returns None"""
    P, k = len(commitments), len(claims)
    n = len(claims[0][1])
    w, s = absorb_and_draw(n, P, claims, proof["evaluations"], t)
    num_vars, claimed_sum, r_polys = proof["sumcheck"]
    if (len(proof["evaluations"]) != k or num_vars != n or len(r_polys) != n
            or any(len(rp) > 3 for rp in r_polys)):
        raise ValueError("Multi-open proof shape mismatch")
    if claimed_sum % R != s:
        raise ValueError("Multi-open claimed sum mismatch")
    r, e = o.SumcheckProof(num_vars, claimed_sum, r_polys).verify(t)
    point, evaluation, s_comm, ops = proof["opening"]
    if list(point) != list(r) or evaluation % R != e % R:
        raise ValueError("Multi-open final evaluation mismatch")
    cstar = None
    for cj, C in zip(combiners(P, claims, w, r), commitments):
        cstar = o.g1_add(cstar, o.g1_mul(C, cj))
    if not o.MLEvalProof(point, evaluation, s_comm, *ops).verify(cstar, kzg, t):
        raise ValueError("Multi-open opening verification failed")


def make_case(n, P, k, seed=None):
    """polys and claims with claim i on polynomial i % P; claim 1 repeats claim
    0's point (on another polynomial when P > 1) and claim 2's point has 0/1
    coordinates"""
    rnd = random.Random(10000 * n + 100 * P + k if seed is None else seed)
    polys = [[rnd.randrange(R) for _ in range(1 << n)] for _ in range(P)]
    claims = [(i % P, [rnd.randrange(R) for _ in range(n)]) for i in range(k)]
    if k >= 2:
        claims[1] = (claims[1][0], list(claims[0][1]))
    if k >= 3:
        claims[2] = (claims[2][0], [rnd.randrange(2) for _ in range(n)])
    return polys, claims


def to_product(q, proof):
    """the plain-data proof as the product's dataclasses"""
    point, evaluation, s_comm, ops = proof["opening"]
    nv, cs, r_polys = proof["sumcheck"]
    return q.MultiOpenProof(list(proof["evaluations"]),
                            q.SumcheckProof(nv, cs, [list(rp) for rp in r_polys]),
                            q.MLEvalProof(list(point), evaluation, s_comm,
                                          *[q.KZGOpeningProof(*op) for op in ops]))


def from_product(p):
    op = p.opening
    return {"evaluations": list(p.evaluations),
            "sumcheck": [p.sumcheck.num_vars, p.sumcheck.claimed_sum,
                         [list(rp) for rp in p.sumcheck.r_polys]],
            "opening": [list(op.evaluation_point), op.evaluation, op.s_comm,
                        [(x.x, x.y, x.proof) for x in (getattr(op, name) for name in OPENINGS)]]}
