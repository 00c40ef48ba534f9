"""InnerProductProof::prove / verify (pcs/src/ipa.rs:59-112, :160-202) restated
on the oracle's primitives, for the tests of the device prover and the host
verifier.  `kzg` is an `o.KZG(max_degree, tau, points=[])`: it commits and
opens through the trapdoor ([p(tau)] g1), and its `verify` is the trapdoor
identity, independent of the product's pairing check.

A proof is a tuple like `o.MLEvalProof`'s openings:
    (inner_product, s_comm, f_opening, f_opening_inv, g_opening, g_opening_inv,
     s_opening, s_opening_inv),    each opening (x, y, pi).
"""
import quill_oracle as o

R = o.R_MOD
OPENINGS = ("f_opening", "f_opening_inv", "g_opening", "g_opening_inv", "s_opening",
            "s_opening_inv")


def equation_holds(inner_product, r, ys) -> bool:
    """ipa.rs:94-100 / :198-201 on the six y values in proof order"""
    yf, yfi, yg, ygi, ys_, ysi = ys
    lhs = yf * ygi + yfi * yg
    rhs = r * ys_ + o.fr_inv(r) * ysi + 2 * inner_product
    return (lhs - rhs) % R == 0


def prove(poly1, poly2, kzg, t):
    """ipa.rs:59-112"""
    inner_product = sum(a * b for a, b in zip(poly1, poly2)) % R
    s_poly = o.compute_s_polynomial(poly1, poly2)
    s_comm = kzg.commit(s_poly)
    t.append_fr(inner_product)
    t.append_g1(s_comm)
    r = t.draw_field_element()
    r_inv = o.fr_inv(r)
    ops = [kzg.open(p, x) for p in (poly1, poly2, s_poly) for x in (r, r_inv)]
    assert equation_holds(inner_product, r, [op[1] for op in ops]), \
        "Inner product verification equation failed"
    return (inner_product, s_comm, *ops)


def verify(proof, comm1, comm2, kzg, t) -> bool:
    """ipa.rs:160-202: the six KZG checks first (a failure returns before the
    transcript is touched), then inner_product, s_comm, r and the equation"""
    inner_product, s_comm = proof[0], proof[1]
    ops = proof[2:]
    for C, op in zip((comm1, comm1, comm2, comm2, s_comm, s_comm), ops):
        if not kzg.verify(C, op):
            return False
    t.append_fr(inner_product)
    t.append_g1(s_comm)
    r = t.draw_field_element()
    return equation_holds(inner_product, r, [op[1] for op in ops])


def to_product(q, proof):
    """the tuple as the product's dataclass"""
    return q.InnerProductProof(proof[0], proof[1], *[q.KZGOpeningProof(*op) for op in proof[2:]])


def from_product(p):
    return (p.inner_product, p.s_comm,
            *[(op.x, op.y, op.proof) for op in (getattr(p, n) for n in OPENINGS)])
