"""Expressions and tables shared by the sumcheck parity tests
(test_gpu_sumcheck_rounds.py on the device, test_oracle_c.py for the C oracle).

Each case names the large-round kernel the prover's dispatch gives it on one
GPU: "pure" (k_sc_big<K,4,true>: a product of distinct tables, at most 4
points), "sop" (k_sc_big<4,4,false>: any other expression of at most 4 tables
and degree at most 3) or "staged" (k_sc_round<K,NP>, with its <K,NP>)."""
import functools
import random
from collections import namedtuple

import quill_oracle as o

R = o.R_MOD

Case = namedtuple("Case", "name ntab degree kernel knp build")


def _prod(I, idx):
    e = I(idx[0])
    for i in idx[1:]:
        e = e * I(i)
    return e


CASES = [
    # k_sc_big<4,4,true>
    Case("prod2", 2, 2, "pure", (4, 4), lambda I, C: _prod(I, [0, 1])),
    Case("prod3", 3, 3, "pure", (4, 4), lambda I, C: _prod(I, [0, 1, 2])),
    Case("prod4", 4, 4, "staged", (4, 8), lambda I, C: _prod(I, [0, 1, 2, 3])),
    # k_sc_big<4,4,false>
    Case("mixed", 4, 3, "sop", (4, 4),
         lambda I, C: C(5) * _prod(I, [0, 1, 2]) + C(R - 7) * I(1) * I(3) - I(2)),
    Case("repeat", 2, 2, "sop", (4, 4), lambda I, C: I(1) * I(1) - I(1)),
    Case("deg1", 2, 1, "sop", (4, 4), lambda I, C: C(3) * I(0) + I(1)),
    Case("const", 1, 0, "sop", (4, 4), lambda I, C: C(0x1234567)),
    Case("const_plus", 3, 2, "sop", (4, 4), lambda I, C: C(9) + I(0) * I(1) + C(4) * I(2)),
    Case("slots13", 4, 3, "sop", (4, 4), lambda I, C: I(1) * I(3) * I(1) + C(3) * I(3)),
    # k_sc_round<8,4>
    Case("k5d3", 5, 3, "staged", (8, 4),
         lambda I, C: _prod(I, [0, 1, 2]) + C(2) * I(3) * I(4) - I(0)),
    Case("k8d3", 8, 3, "staged", (8, 4),
         lambda I, C: _prod(I, [0, 1, 2]) + _prod(I, [3, 4, 5]) - I(6) * I(7)),
    # k_sc_round<4,8>
    Case("k4d4", 4, 4, "staged", (4, 8),
         lambda I, C: _prod(I, [0, 1, 2, 3]) + C(3) * I(1) * I(2) - I(0)),
    Case("k4d7", 4, 7, "staged", (4, 8),
         lambda I, C: _prod(I, [0, 0, 1, 1, 2, 2, 3]) + C(5) * I(0) * I(3) + I(2)),
    # k_sc_round<8,8>
    Case("k8d5", 8, 5, "staged", (8, 8),
         lambda I, C: _prod(I, [0, 1, 2, 3, 4]) + C(3) * _prod(I, [5, 6, 7]) - I(0) * I(7)),
    # k_sc_round<8,16>
    Case("k3d9", 3, 9, "staged", (8, 16),
         lambda I, C: _prod(I, [0, 1, 2] * 3) + C(2) * I(0)),
    Case("k8d12", 8, 12, "staged", (8, 16),
         lambda I, C: _prod(I, [0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3]) + C(7) * I(4) * I(5)),
    # every monomial holds table 0 (an all-zero table 0 empties every message)
    Case("fac_sop", 4, 3, "sop", (4, 4),
         lambda I, C: C(5) * _prod(I, [0, 1, 2]) + C(R - 7) * I(0) * I(3)),
    Case("fac_k4d4", 4, 4, "staged", (4, 8),
         lambda I, C: _prod(I, [0, 1, 2, 3]) + C(3) * _prod(I, [0, 1, 2])),
]
BY_NAME = {c.name: c for c in CASES}


def oracle_expr(case):
    return case.build(o.Expr.input, o.Expr.const)


@functools.lru_cache(maxsize=None)
def tables(nvars, ntab, seed=0):
    """ntab tables of 2^nvars uniform field elements (tuples: shared, read-only)"""
    rnd = random.Random(1000003 * seed + 97 * nvars + ntab)
    return tuple(tuple(rnd.randrange(R) for _ in range(1 << nvars)) for _ in range(ntab))


def true_sum(case, tabs):
    e = oracle_expr(case)
    return sum(e.evaluate(g) for g in zip(*tabs)) % R


def oracle_prove(nvars, tabs, expr, claimed, label):
    """o.SumcheckProof.prove_fast -> (r_polys, point, evaluation, transcript state)"""
    st = o.VirtualPolynomialStore(nvars)
    for t in tabs:
        st.allocate_polynomial(list(t))
    h = st.new_virtual_from_expr(expr)
    tr = o.Transcript(label)
    proof, (pt, ev) = o.SumcheckProof.prove_fast(nvars, st, h, claimed, tr)
    return proof.r_polys, pt, ev, tr.state


def degenerate_tables(kind, nvars, ntab, seed=3):
    """Tables that make round messages shorter than degree + 1 (DensePolynomial
    trims trailing zeros; the length goes into the transcript):
      zero_factor   table 0 is all zero
      const_bit0    every table is constant in index bit 0 (round 0 sums constants)
      const_bits01  ... in index bits 0 and 1
      small_values  entries from {0, 1, r - 1}
      false_claim   ordinary tables (the caller passes a wrong claimed sum)"""
    base = [list(t) for t in tables(nvars, ntab, seed)]
    n = 1 << nvars
    if kind == "zero_factor":
        base[0] = [0] * n
    elif kind == "const_bit0":
        base = [[t[i & ~1] for i in range(n)] for t in base]
    elif kind == "const_bits01":
        base = [[t[i & ~3] for i in range(n)] for t in base]
    elif kind == "small_values":
        base = [[(0, 1, R - 1)[x % 3] for x in t] for t in base]
    else:
        assert kind == "false_claim"
    return tuple(tuple(t) for t in base)
