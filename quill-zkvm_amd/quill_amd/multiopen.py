"""Multi-point batch opening (HyperPlonk paper, section 3.8): k evaluation
claims f_{j_i}(z_i) = y_i over P committed multilinear polynomials become one
sumcheck and ONE ML-PCS opening.  No counterpart in the reference; composed
here over the C-ABI like the Logup PIOPs (logup.py).

With t drawn after the claims are absorbed and w_i = t^i,

    s = sum_i w_i y_i = sum_x sum_j g_j(x) f_j(x),
    g_j = sum_{i: j_i = j} w_i eq(., z_i)                 (qg_eq_multi_dev)

is proven by a sumcheck of h = sum_j f_j g_j.  Its final claim (r, e) is
e = sum_j c_j f_j(r) with c_j = g_j(r) = sum_{i: j_i = j} w_i eq(r, z_i), which
the verifier computes itself; f* = sum_j c_j f_j (qg_lincomb_dev) is opened at
r, and the commitment being linear, the verifier checks that opening against
C* = sum_j c_j C_j (qg_g1_lincomb).

Transcript: n, P, k as u64; per claim j_i (u64), z_i (Fr vector), y_i; draw t;
SumcheckProof's absorbs; MLEvalProof's absorbs."""
from __future__ import annotations

from dataclasses import dataclass

from .field import R_MOD, eq_eval
from .hyperplonk import SumcheckProof, VirtualPolyExpr, VirtualPolynomialStore
from .pcs import MLEvalProof, g1_lincomb
from .transcript import Transcript


def _absorb_and_draw(n, P, claims, evaluations, transcript: Transcript):
    """the claims into the transcript; -> (weights w_i = t^i, s = sum w_i y_i)"""
    transcript.append_u64(n)
    transcript.append_u64(P)
    transcript.append_u64(len(claims))
    for (j, z), y in zip(claims, evaluations):
        transcript.append_u64(j)
        transcript.append_fr_vec(list(z))
        transcript.append_fr(y)
    t = transcript.draw_field_element()
    w, acc = [], 1
    for _ in claims:
        w.append(acc)
        acc = acc * t % R_MOD
    return w, sum(wi * y for wi, y in zip(w, evaluations)) % R_MOD


def _combiners(P, claims, w, r):
    """c_j = sum_{i: j_i = j} w_i eq(r, z_i)"""
    c = [0] * P
    for (j, z), wi in zip(claims, w):
        c[j] = (c[j] + wi * eq_eval(list(r), list(z))) % R_MOD
    return c


@dataclass
class MultiOpenProof:
    evaluations: list          # y_i, in claim order
    sumcheck: SumcheckProof
    opening: MLEvalProof       # of sum_j c_j f_j at the sumcheck point

    @staticmethod
    def prove(polys, claims, pcs, transcript: Transcript) -> "MultiOpenProof":
        """polys: P DeviceVec of 2^n entries each, whose commitments are in the
        transcript or fixed before it (as for MLEvalProof::prove, mlpcs.rs:82);
        claims: [(j_i, z_i)] with z_i in Fr^n, at least one per polynomial.
        Up to P = 4 the sumcheck runs on the compiled kernels (2P <= 8 tables);
        beyond that the library's expression interpreter takes it (slower, the
        same proof).  Single-context devices only."""
        dev = pcs.dev
        if dev.world > 1 or dev.comm_info()["sharded"]:
            raise ValueError("MultiOpenProof.prove: not supported on a sharded device")
        P, k = len(polys), len(claims)
        n = len(claims[0][1])
        N = 1 << n
        assert all(len(f) == N for f in polys), "polynomial length is not 2^n"
        assert all(0 <= j < P and len(z) == n for j, z in claims), "malformed claim"
        by_poly = [[i for i, (j, _) in enumerate(claims) if j == jj] for jj in range(P)]
        assert all(by_poly), "a polynomial without a claim"
        claims = [(j, [int(c) % R_MOD for c in z]) for j, z in claims]
        evaluations = [0] * k
        for jj, idx in enumerate(by_poly):
            for i, y in zip(idx, dev.mle_eval_multi(polys[jj], [claims[i][1] for i in idx])):
                evaluations[i] = y
        w, s = _absorb_and_draw(n, P, claims, evaluations, transcript)
        gs = [dev.eq_multi_dev([claims[i][1] for i in idx], [w[i] for i in idx])
              for idx in by_poly]
        store = VirtualPolynomialStore(n, dev)
        for f in polys:
            store.allocate_polynomial(f)
        for g in gs:
            store.allocate_polynomial(g)
        E = VirtualPolyExpr
        h = E.Input(0) * E.Input(P)
        for j in range(1, P):
            h = h + E.Input(j) * E.Input(P + j)
        sumcheck, claim = SumcheckProof.prove(n, store, store.new_virtual_from_expr(h), s,
                                              transcript)
        fstar = dev.lincomb_dev(polys, _combiners(P, claims, w, claim.point), N)
        opening = pcs.open_dev(fstar, N, claim.point, transcript)
        for v in gs + [fstar]:
            v.close()
        assert opening.evaluation == claim.evaluation, "multi-open final evaluation mismatch"
        return MultiOpenProof(evaluations, sumcheck, opening)

    def verify(self, commitments, claims, pcs, transcript: Transcript) -> None:
        """commitments: the P commitments C_j; claims: [(j_i, z_i)] as the
        verifier derives them (the claimed values are self.evaluations).
        Raises ValueError; host code (pcs may be a deferring view, which then
        collects the opening's four KZG claims)."""
        P, k = len(commitments), len(claims)
        n = len(claims[0][1]) if claims else 0
        assert all(0 <= j < P and len(z) == n for j, z in claims), "malformed claim"
        w, s = _absorb_and_draw(n, P, claims, self.evaluations, transcript)
        sc = self.sumcheck
        # SumcheckProof.verify checks neither the number of rounds nor a degree
        if (len(self.evaluations) != k or sc.num_vars != n or len(sc.r_polys) != n
                or any(len(rp) > 3 for rp in sc.r_polys)):
            raise ValueError("Multi-open proof shape mismatch")
        if sc.claimed_sum % R_MOD != s:
            raise ValueError("Multi-open claimed sum mismatch")
        claim = sc.verify(transcript)
        if (self.opening.point() != list(claim.point)
                or self.opening.evaluation % R_MOD != claim.evaluation % R_MOD):
            raise ValueError("Multi-open final evaluation mismatch")
        cstar = g1_lincomb(list(commitments), _combiners(P, claims, w, claim.point))
        if not pcs.verify(cstar, self.opening, transcript):
            raise ValueError("Multi-open opening verification failed")
