"""The folded ML opening restated on the oracle's primitives alone, prover and
verifier, for the tests of the device prover and of the product's host
verifiers.  `kzg` is an `o.KZG(max_degree, tau, points=[])`: it commits through
the trapdoor and verifies by the trapdoor identity.

An MLEvalProof opens f and S, each at r and 1/r.  Two polynomials opened at
the same point need one quotient:
  1. as MLEvalProof::prove: evaluation, S, s_comm; append point, evaluation,
     s_comm; draw r (r != 0)
  2. y = (f(r), f(1/r), S(r), S(1/r)); append the four as Fr in that order;
     draw gamma (not redrawn when 0); nothing further is absorbed
  3. h = f + gamma S, a missing coefficient of the shorter operand counting as
     0, over L_h = max(trimmed length of f, of S) coefficients;
     w = commit((h - h(r))/(X - r)), w_inv the same at 1/r
  4. the verifier replays 1 and 2, checks the inner-product equation on the
     four y, forms C_h = C_f + gamma s_comm and checks the two KZG claims
     (C_h, r, y0 + gamma y2, w) and (C_h, 1/r, y1 + gamma y3, w_inv)

A proof is plain data, so a test can copy and tamper with it:
    {"point": [..], "evaluation": e, "s_comm": P, "y": [y0, y1, y2, y3],
     "w": P, "w_inv": P}"""
import quill_oracle as o

R = o.R_MOD
Y_FIELDS = ("y_poly", "y_poly_inv", "y_s", "y_s_inv")


def challenges(point, evaluation, s_comm, y, t):
    """the transcript of steps 1 and 2 -> (r, 1/r, gamma)"""
    t.append_fr_vec(list(point))
    t.append_fr(evaluation)
    t.append_g1(s_comm)
    r = t.draw_field_element()
    assert r != 0, "challenge r = 0"
    for v in y:
        t.append_fr(v)
    return r, o.fr_inv(r), t.draw_field_element()


def fold(f, s, gamma):
    """h = f + gamma S over max(trimmed lengths) coefficients (untrimmed itself)"""
    f, s = o.poly_trim(list(f)), o.poly_trim(list(s))
    L = max(len(f), len(s))
    f, s = f + [0] * (L - len(f)), s + [0] * (L - len(s))
    return [(a + gamma * b) % R for a, b in zip(f, s)]


def quotient_commit(h, x, kzg):
    """commit((h - h(x))/(X - x)) over len(h) - 1 coefficients, and h(x)"""
    assert len(h) - 1 <= kzg.max_degree + 1, "Polynomial degree exceeds max degree"
    q, y = o.poly_div_linear(h, x)  # trims: zero tail coefficients commit to nothing
    return kzg.commit(q), y


def prove(poly, point, kzg, t):
    pr = o.compute_pr(point)
    evaluation = sum(a * b for a, b in zip(poly, pr)) % R
    s_poly = o.compute_s_polynomial(poly, pr)
    s_comm = kzg.commit(s_poly)
    t.append_fr_vec(list(point))
    t.append_fr(evaluation)
    t.append_g1(s_comm)
    r = t.draw_field_element()
    assert r != 0, "challenge r = 0"
    r_inv = o.fr_inv(r)
    # the four values are bound before the challenge that folds them
    y = [o.poly_eval(poly, r), o.poly_eval(poly, r_inv),
         o.poly_eval(s_poly, r), o.poly_eval(s_poly, r_inv)]
    for v in y:
        t.append_fr(v)
    gamma = t.draw_field_element()
    h = fold(poly, s_poly, gamma)
    w, yh = quotient_commit(h, r, kzg)
    w_inv, yh_inv = quotient_commit(h, r_inv, kzg)
    assert yh == (y[0] + gamma * y[2]) % R and yh_inv == (y[1] + gamma * y[3]) % R
    return {"point": list(point), "evaluation": evaluation, "s_comm": s_comm, "y": y,
            "w": w, "w_inv": w_inv}


def verify(proof, commitment, kzg, t) -> bool:
    """the transcript always advances to the prover's final state"""
    y = [v % R for v in proof["y"]]
    r, r_inv, gamma = challenges(proof["point"], proof["evaluation"], proof["s_comm"], y, t)
    c_h = o.g1_add(commitment, o.g1_mul(proof["s_comm"], gamma))
    if not kzg.verify(c_h, (r, (y[0] + gamma * y[2]) % R, proof["w"])):
        return False
    if not kzg.verify(c_h, (r_inv, (y[1] + gamma * y[3]) % R, proof["w_inv"])):
        return False
    pr_r, pr_r_inv = o.eval_pr(proof["point"], r), o.eval_pr(proof["point"], r_inv)
    lhs = y[0] * pr_r_inv + y[1] * pr_r
    rhs = r * y[2] + r_inv * y[3] + 2 * proof["evaluation"]
    return (lhs - rhs) % R == 0


def gamma_of(proof, t):
    """the honest gamma of a proof from the transcript state before it"""
    return challenges(proof["point"], proof["evaluation"], proof["s_comm"], proof["y"], t.clone())[2]


def to_product(q, proof):
    """the plain-data proof as the product's dataclass"""
    return q.FoldedMLEvalProof(list(proof["point"]), proof["evaluation"], proof["s_comm"],
                               *proof["y"], proof["w"], proof["w_inv"])


def from_product(p):
    return {"point": list(p.evaluation_point), "evaluation": p.evaluation, "s_comm": p.s_comm,
            "y": [getattr(p, n) for n in Y_FIELDS], "w": p.w, "w_inv": p.w_inv}
