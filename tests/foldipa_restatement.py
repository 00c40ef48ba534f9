"""The folded inner-product argument restated on the oracle's primitives alone,
prover and verifier, for the tests of the device prover and of the product's
host verifiers.  `kzg` is an `o.KZG(max_degree, tau, points=[])`: it commits
through the trapdoor and verifies by the trapdoor identity.

InnerProductProof::prove opens f, g and S, each at r and 1/r (ipa.rs:86-92).
Three polynomials opened at the same point need one quotient:
  1. as ipa.rs:59-83: inner_product over the common prefix, S of the
     zero-padded pair, s_comm over the trimmed S; append inner_product, then
     s_comm; draw r (r != 0)
  2. y = (f(r), f(1/r), g(r), g(1/r), S(r), S(1/r)); append the six as Fr in
     that order; draw gamma (not redrawn when 0); nothing further is absorbed;
     the prover asserts ipa.rs:94-100 on the six y
  3. h = f + gamma g + gamma^2 S, a missing coefficient counting as 0, over
     L_h = max(trimmed lengths of f, g, S) coefficients;
     w = commit((h - h(r))/(X - r)), w_inv the same at 1/r
  4. the verifier replays 1 and 2 (so the transcript always advances), forms
     C_h = C_f + gamma C_g + gamma^2 s_comm, checks the two KZG claims
     (C_h, r, y0 + gamma y2 + gamma^2 y4, w) and
     (C_h, 1/r, y1 + gamma y3 + gamma^2 y5, w_inv), and the equation on the six y

A proof is plain data, so a test can copy and tamper with it:
    {"inner_product": v, "s_comm": P, "y": [y0, .., y5], "w": P, "w_inv": P}"""
import quill_oracle as o

R = o.R_MOD
Y_FIELDS = ("y_f", "y_f_inv", "y_g", "y_g_inv", "y_s", "y_s_inv")


def equation_holds(inner_product, r, y) -> bool:
    """ipa.rs:94-100 / :198-201 on the six y"""
    lhs = y[0] * y[3] + y[1] * y[2]
    rhs = r * y[4] + o.fr_inv(r) * y[5] + 2 * inner_product
    return (lhs - rhs) % R == 0


def _mul(a, b):
    """the exact integer product of two coefficient lists through one big-integer
    multiplication (Kronecker substitution): a coefficient of the product is a
    sum of at most min(len) products of two values < 2^254, so < 2^540 for any
    length below 2^32 and the 544-bit slots never carry into each other"""
    if not a or not b:
        return []
    W = 544
    A = sum(x << (W * i) for i, x in enumerate(a))
    B = sum(x << (W * i) for i, x in enumerate(b))
    C, mask = A * B, (1 << W) - 1
    return [(C >> (W * i)) & mask for i in range(len(a) + len(b) - 1)]


def s_polynomial(f, g):
    """o.compute_s_polynomial (ipa.rs:122-157) with the two products by _mul:
    the oracle's schoolbook product takes seconds at 2049 coefficients.  The
    CPU test compares the two at its lengths."""
    M = max(len(f), len(g))
    f = [x % R for x in f] + [0] * (M - len(f))
    g = [x % R for x in g] + [0] * (M - len(g))
    if M == 0:
        return []
    h = [(a + b) % R for a, b in zip(_mul(f, g[::-1]), _mul(f[::-1], g))]
    return o.poly_trim(h[(len(h) // 2 + 1):])


def challenges(inner_product, s_comm, y, t):
    """the transcript of steps 1 and 2 -> (r, 1/r, gamma)"""
    t.append_fr(inner_product)
    t.append_g1(s_comm)
    r = t.draw_field_element()
    assert r != 0, "challenge r = 0"
    for v in y:
        t.append_fr(v)
    return r, o.fr_inv(r), t.draw_field_element()


def fold(polys, gamma):
    """h = sum_q gamma^q polys[q] over max(trimmed lengths) coefficients"""
    ps = [o.poly_trim(list(p)) for p in polys]
    L = max(len(p) for p in ps)
    h, gq = [0] * L, 1
    for p in ps:
        for i, c in enumerate(p):
            h[i] = (h[i] + gq * c) % R
        gq = gq * gamma % R
    return h


def quotient_commit(h, x, kzg):
    """commit((h - h(x))/(X - x)) over len(h) - 1 coefficients, and h(x)"""
    assert len(h) - 1 <= kzg.max_degree + 1, "Polynomial degree exceeds max degree"
    q, y = o.poly_div_linear(h, x)  # trims: zero tail coefficients commit to nothing
    return kzg.commit(q), y


def prove(poly1, poly2, kzg, t):
    assert len(poly1) or len(poly2)
    inner_product = sum(a * b for a, b in zip(poly1, poly2)) % R
    s_poly = s_polynomial(poly1, poly2)
    s_comm = kzg.commit(s_poly)
    t.append_fr(inner_product)
    t.append_g1(s_comm)
    r = t.draw_field_element()
    assert r != 0, "challenge r = 0"
    r_inv = o.fr_inv(r)
    # the six values are bound before the challenge that folds them
    y = [o.poly_eval(p, x) for p in (poly1, poly2, s_poly) for x in (r, r_inv)]
    assert equation_holds(inner_product, r, y), "Inner product verification equation failed"
    for v in y:
        t.append_fr(v)
    gamma = t.draw_field_element()
    h = fold((poly1, poly2, s_poly), gamma)
    w, yh = quotient_commit(h, r, kzg)
    w_inv, yh_inv = quotient_commit(h, r_inv, kzg)
    g2 = gamma * gamma % R
    assert yh == (y[0] + gamma * y[2] + g2 * y[4]) % R
    assert yh_inv == (y[1] + gamma * y[3] + g2 * y[5]) % R
    return {"inner_product": inner_product, "s_comm": s_comm, "y": y, "w": w, "w_inv": w_inv}


def verify(proof, comm1, comm2, kzg, t) -> bool:
    """the transcript always advances to the prover's final state"""
    y = [v % R for v in proof["y"]]
    r, r_inv, gamma = challenges(proof["inner_product"], proof["s_comm"], y, t)
    g2 = gamma * gamma % R
    c_h = o.g1_add(o.g1_add(comm1, o.g1_mul(comm2, gamma)), o.g1_mul(proof["s_comm"], g2))
    if not kzg.verify(c_h, (r, (y[0] + gamma * y[2] + g2 * y[4]) % R, proof["w"])):
        return False
    if not kzg.verify(c_h, (r_inv, (y[1] + gamma * y[3] + g2 * y[5]) % R, proof["w_inv"])):
        return False
    return equation_holds(proof["inner_product"], r, y)


def gamma_of(proof, t):
    """the honest gamma of a proof from the transcript state before it"""
    return challenges(proof["inner_product"], proof["s_comm"], proof["y"], t.clone())[2]


def to_product(q, proof):
    """the plain-data proof as the product's dataclass"""
    return q.FoldedInnerProductProof(proof["inner_product"], proof["s_comm"], *proof["y"],
                                     proof["w"], proof["w_inv"])


def from_product(p):
    return {"inner_product": p.inner_product, "s_comm": p.s_comm,
            "y": [getattr(p, n) for n in Y_FIELDS], "w": p.w, "w_inv": p.w_inv}
