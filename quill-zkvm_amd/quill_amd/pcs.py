"""PCS mirror: KZG (pcs/src/kzg.rs), MLEvalProof (pcs/src/mlpcs.rs) and the
MultilinearPCS trait surface (pcs/src/lib.rs:26-41), backed by the gfx950
kernels through the C-ABI.  Field elements are canonical Python ints; G1 points
are affine (x, y) tuples or None (infinity)."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from ._lib import (IpaProof, IpaProofFolded, KzgClaim, KzgOpening, KzgVk, MleOpenItem, MleProof,
                   MleProofFolded, QuillGpuError, check, lib)
from .device import Device, DeviceVec, Srs
from .field import (fq_from_mont_limbs, fr_array, fr_c, fr_from_mont_limbs, g1_from_abi,
                    g1_to_abi, g2_from_abi, g2_to_abi, u64p)
from .transcript import Transcript


@dataclass
class EvaluationClaim:
    """pcs/src/lib.rs:10-13"""
    point: list
    evaluation: int


@dataclass
class KZGOpeningProof:
    """pcs/src/kzg.rs:25-32"""
    x: int
    y: int
    proof: object


def _opening_c(o: KZGOpeningProof) -> KzgOpening:
    c = KzgOpening()
    C.memmove(c.x, fr_c(o.x), 32)
    C.memmove(c.y, fr_c(o.y), 32)
    xy, inf = g1_to_abi(o.proof)
    C.memmove(c.proof_xy, xy, 64)
    c.proof_inf = inf
    return c


def _mle_proof_c(p: "MLEvalProof") -> MleProof:
    c = MleProof()
    C.memmove(c.evaluation, fr_c(p.evaluation), 32)
    xy, inf = g1_to_abi(p.s_comm)
    C.memmove(c.s_comm_xy, xy, 64)
    c.s_comm_inf = inf
    c.poly_opening = _opening_c(p.poly_opening)
    c.poly_opening_inv = _opening_c(p.poly_opening_inv)
    c.s_opening = _opening_c(p.s_opening)
    c.s_opening_inv = _opening_c(p.s_opening_inv)
    return c


# ---------------------------------------------------------------- pairing group G2
G1_GENERATOR = (1, 2)


def g2_generator():
    """ark-bn254 G2Affine::generator() as ((x0, x1), (y0, y1))"""
    xy = (C.c_uint64 * 16)()
    check(lib().qg_g2_generator(xy))
    return g2_from_abi(xy, 0)


def g2_mul(Q, k: int):
    xy, inf = g2_to_abi(Q)
    out, oinf = (C.c_uint64 * 16)(), C.c_uint8()
    check(lib().qg_g2_mul(xy, inf, fr_c(k), out, C.byref(oinf)))
    return g2_from_abi(out, oinf.value)


def g1_lincomb(points, scalars):
    """sum_i scalars[i] points[i] on the host (qg_g1_lincomb): the combined
    commitment of a batch opening.  None is the identity, as input and result."""
    n = len(points)
    assert n == len(scalars) and n >= 1
    xy = np.zeros((n, 8), dtype=np.uint64)
    inf = np.zeros(n, dtype=np.uint8)
    for i, pt in enumerate(points):
        a, f = g1_to_abi(pt)
        xy[i, :] = list(a)
        inf[i] = f
    out, oinf = (C.c_uint64 * 8)(), C.c_uint8()
    check(lib().qg_g1_lincomb(u64p(xy), inf.ctypes.data_as(C.POINTER(C.c_uint8)),
                              u64p(fr_array(scalars)), n, out, C.byref(oinf)))
    return g1_from_abi(out, oinf.value)


def pairing(P, Q):
    """E::pairing(P, Q) (ark-bn254 optimal ate) in the tower layout of
    qg_pairing: 12 canonical Fq ints (c0.c0.re, c0.c0.im, c0.c1.re, ...)"""
    pxy, pinf = g1_to_abi(P)
    qxy, qinf = g2_to_abi(Q)
    out = (C.c_uint64 * 48)()
    check(lib().qg_pairing(pxy, pinf, qxy, qinf, out))
    return [fq_from_mont_limbs(list(out)[4 * k:4 * k + 4]) for k in range(12)]


def _opening(o: KzgOpening) -> KZGOpeningProof:
    return KZGOpeningProof(fr_from_mont_limbs(list(o.x)), fr_from_mont_limbs(list(o.y)),
                           g1_from_abi(o.proof_xy, o.proof_inf))


@dataclass
class MLEvalProof:
    """pcs/src/mlpcs.rs:32-44"""
    evaluation_point: list
    evaluation: int
    s_comm: object
    poly_opening: KZGOpeningProof
    poly_opening_inv: KZGOpeningProof
    s_opening: KZGOpeningProof
    s_opening_inv: KZGOpeningProof

    def verify(self, commitment, kzg: "KZG", transcript: Transcript) -> bool:
        """mlpcs.rs:126-161 (host pairing check, qg_mle_verify)"""
        return kzg.verify(commitment, self, transcript)

    # MultilinearPCSProof (pcs/src/lib.rs:15-24)
    def point(self):
        return list(self.evaluation_point)

    def evaluation_claim(self):
        return EvaluationClaim(self.point(), self.evaluation)


@dataclass
class FoldedMLEvalProof:
    """The folded ML opening (no counterpart in the reference; DESIGN section
    5): f and S are opened at the same two points r and 1/r, so one quotient
    per point, of f + gamma S, serves both.  y_* are the four values the
    transcript absorbs before gamma is drawn; w, w_inv the two quotient
    commitments.  The verifier derives the opening points and folded values."""
    evaluation_point: list
    evaluation: int
    s_comm: object
    y_poly: int
    y_poly_inv: int
    y_s: int
    y_s_inv: int
    w: object
    w_inv: object

    def verify(self, commitment, kzg: "KZG", transcript: Transcript) -> bool:
        """qg_mle_verify_folded (or two claims of a deferring view's batch)"""
        return kzg.verify(commitment, self, transcript)

    def point(self):
        return list(self.evaluation_point)

    def evaluation_claim(self):
        return EvaluationClaim(self.point(), self.evaluation)


_FOLDED_Y = ("y_poly", "y_poly_inv", "y_s", "y_s_inv")
_FOLDED_CLAIMS = ("folded at r", "folded at 1/r")


def _folded_proof_c(p: FoldedMLEvalProof) -> MleProofFolded:
    c = MleProofFolded()
    C.memmove(c.evaluation, fr_c(p.evaluation), 32)
    for fld, pt in (("s_comm", p.s_comm), ("w", p.w), ("w_inv", p.w_inv)):
        xy, inf = g1_to_abi(pt)
        C.memmove(getattr(c, fld + "_xy"), xy, 64)
        setattr(c, fld + "_inf", inf)
    for i, name in enumerate(_FOLDED_Y):
        C.memmove(c.y[i], fr_c(getattr(p, name)), 32)
    return c


def _folded_proof(pt, o: MleProofFolded) -> FoldedMLEvalProof:
    return FoldedMLEvalProof(list(pt), fr_from_mont_limbs(list(o.evaluation)),
                             g1_from_abi(o.s_comm_xy, o.s_comm_inf),
                             *[fr_from_mont_limbs(list(o.y[i])) for i in range(4)],
                             g1_from_abi(o.w_xy, o.w_inf), g1_from_abi(o.w_inv_xy, o.w_inv_inf))


def _ipa_proof_c(p: "InnerProductProof") -> IpaProof:
    c = IpaProof()
    C.memmove(c.inner_product, fr_c(p.inner_product), 32)
    xy, inf = g1_to_abi(p.s_comm)
    C.memmove(c.s_comm_xy, xy, 64)
    c.s_comm_inf = inf
    for name in _IPA_OPENINGS:
        setattr(c, name, _opening_c(getattr(p, name)))
    return c


_IPA_OPENINGS = ("f_opening", "f_opening_inv", "g_opening", "g_opening_inv", "s_opening",
                 "s_opening_inv")


@dataclass
class InnerProductProof:
    """pcs/src/ipa.rs:40-53: <f, g> over the common prefix of two committed
    coefficient vectors, by the S polynomial and six KZG openings at r, 1/r"""
    inner_product: int
    s_comm: object
    f_opening: KZGOpeningProof
    f_opening_inv: KZGOpeningProof
    g_opening: KZGOpeningProof
    g_opening_inv: KZGOpeningProof
    s_opening: KZGOpeningProof
    s_opening_inv: KZGOpeningProof

    @classmethod
    def prove(cls, poly1, poly2, kzg: "KZG", transcript: Transcript) -> "InnerProductProof":
        """ipa.rs:59-112 (qg_ipa_prove; qg_ipa_prove_dev when both operands are
        DeviceVecs).  Like the reference, the commitments to poly1 and poly2
        are the caller's to absorb into the transcript beforehand.
        On a Device with a communicator the operands are this rank's DeviceVec
        blocks of equal length L (world * L a power of two) and `kzg` wraps the
        SRS shard at offset rank * L, as for KZG.open_dev; every rank gets the
        single-context proof.  Host or mixed operands there raise the
        library's error (the host-pointer entry stays single-context)."""
        out = IpaProof()
        dev = kzg.dev
        if isinstance(poly1, DeviceVec) and isinstance(poly2, DeviceVec):
            rc = lib().qg_ipa_prove_dev(dev.h, kzg.srs_for(max(len(poly1), len(poly2))).h,
                                        poly1.h, len(poly1), poly2.h, len(poly2),
                                        transcript.c_state(), C.byref(out))
        else:
            if isinstance(poly1, DeviceVec) or isinstance(poly2, DeviceVec):
                raise QuillGpuError(-1, "InnerProductProof.prove: both operands on the device, "
                                        "or both on the host")
            a = fr_array(poly1) if len(poly1) else np.zeros((1, 4), dtype=np.uint64)
            b = fr_array(poly2) if len(poly2) else np.zeros((1, 4), dtype=np.uint64)
            rc = lib().qg_ipa_prove(dev.h, kzg.srs_for(max(len(poly1), len(poly2))).h, u64p(a),
                                    len(poly1), u64p(b), len(poly2), transcript.c_state(),
                                    C.byref(out))
        check(rc, dev.h)
        return cls(fr_from_mont_limbs(list(out.inner_product)),
                   g1_from_abi(out.s_comm_xy, out.s_comm_inf),
                   *[_opening(getattr(out, name)) for name in _IPA_OPENINGS])

    def verify(self, comm1, comm2, kzg: "KZG", transcript: Transcript) -> bool:
        """ipa.rs:160-202 (host pairing checks, qg_ipa_verify): the six KZG
        checks first - a failure leaves the transcript untouched -, then the
        transcript replay and the equation at r.  With a deferring view
        (KZG.deferring) the six openings become claims of the view's batch, the
        transcript always advances and only the equation's verdict returns."""
        if isinstance(kzg, DeferringKZG):
            return kzg.verify_inner_product(comm1, comm2, self, transcript)
        xy1, inf1 = g1_to_abi(comm1)
        xy2, inf2 = g1_to_abi(comm2)
        ok = C.c_int()
        check(lib().qg_ipa_verify(C.byref(kzg._vk()), xy1, inf1, xy2, inf2,
                                  C.byref(_ipa_proof_c(self)), transcript.c_state(),
                                  C.byref(ok)))
        return bool(ok.value)


_IPA_FOLDED_Y = ("y_f", "y_f_inv", "y_g", "y_g_inv", "y_s", "y_s_inv")


@dataclass
class FoldedInnerProductProof:
    """The folded inner-product argument (no counterpart in the reference;
    DESIGN section 5): f, g and S are opened at the same two points r and 1/r,
    so one quotient per point, of f + gamma g + gamma^2 S, serves all three.
    y_* are the six values the transcript absorbs before gamma is drawn; w,
    w_inv the two quotient commitments.  The verifier derives the opening
    points and folded values."""
    inner_product: int
    s_comm: object
    y_f: int
    y_f_inv: int
    y_g: int
    y_g_inv: int
    y_s: int
    y_s_inv: int
    w: object
    w_inv: object

    @classmethod
    def prove(cls, poly1, poly2, kzg, transcript: Transcript) -> "FoldedInnerProductProof":
        """qg_ipa_prove_folded_dev when both operands are DeviceVecs, else
        qg_ipa_prove_folded on two host vectors; `kzg` is a KZG or its
        FoldingKZG view.  Like InnerProductProof.prove, the commitments to
        poly1 and poly2 are the caller's to absorb beforehand.  Single-context
        only: a Device with a communicator raises ValueError."""
        dev = kzg.dev
        if dev.world > 1 or dev.comm_info()["sharded"]:
            raise ValueError("the folded inner-product argument is not supported on a sharded "
                             "device (communicator attached)")
        out = IpaProofFolded()
        n = max(len(poly1), len(poly2))
        if isinstance(poly1, DeviceVec) and isinstance(poly2, DeviceVec):
            rc = lib().qg_ipa_prove_folded_dev(dev.h, kzg.srs_for(n).h, poly1.h, len(poly1),
                                               poly2.h, len(poly2), transcript.c_state(),
                                               C.byref(out))
        else:
            if isinstance(poly1, DeviceVec) or isinstance(poly2, DeviceVec):
                raise QuillGpuError(-1, "FoldedInnerProductProof.prove: both operands on the "
                                        "device, or both on the host")
            a = fr_array(poly1) if len(poly1) else np.zeros((1, 4), dtype=np.uint64)
            b = fr_array(poly2) if len(poly2) else np.zeros((1, 4), dtype=np.uint64)
            rc = lib().qg_ipa_prove_folded(dev.h, kzg.srs_for(n).h, u64p(a), len(poly1), u64p(b),
                                           len(poly2), transcript.c_state(), C.byref(out))
        check(rc, dev.h)
        return cls(fr_from_mont_limbs(list(out.inner_product)),
                   g1_from_abi(out.s_comm_xy, out.s_comm_inf),
                   *[fr_from_mont_limbs(list(out.y[i])) for i in range(6)],
                   g1_from_abi(out.w_xy, out.w_inf), g1_from_abi(out.w_inv_xy, out.w_inv_inf))

    def verify(self, comm1, comm2, kzg, transcript: Transcript) -> bool:
        """qg_ipa_verify_folded: the transcript is replayed first (gamma comes
        from it) and always advances to the prover's final state, whatever the
        verdict.  With a deferring view (KZG.deferring) the two claims join the
        view's batch and only the equation's verdict returns."""
        if isinstance(kzg, DeferringKZG):
            return kzg.verify_inner_product(comm1, comm2, self, transcript)
        xy1, inf1 = g1_to_abi(comm1)
        xy2, inf2 = g1_to_abi(comm2)
        ok = C.c_int()
        check(lib().qg_ipa_verify_folded(C.byref(kzg._vk()), xy1, inf1, xy2, inf2,
                                         C.byref(_ipa_folded_proof_c(self)),
                                         transcript.c_state(), C.byref(ok)))
        return bool(ok.value)


def _ipa_folded_proof_c(p: FoldedInnerProductProof) -> IpaProofFolded:
    c = IpaProofFolded()
    C.memmove(c.inner_product, fr_c(p.inner_product), 32)
    for fld, pt in (("s_comm", p.s_comm), ("w", p.w), ("w_inv", p.w_inv)):
        xy, inf = g1_to_abi(pt)
        C.memmove(getattr(c, fld + "_xy"), xy, 64)
        setattr(c, fld + "_inf", inf)
    for i, name in enumerate(_IPA_FOLDED_Y):
        C.memmove(c.y[i], fr_c(getattr(p, name)), 32)
    return c


class KZG:
    """KZG<Bn254> with a device-resident SRS.

    trusted_setup(max_degree, tau) builds g1_points = [tau^i] g on the device
    (kzg.rs:35-59 with an explicit tau instead of an rng; MultilinearPCS's
    thread_rng setup (mlpcs.rs:178-182) is not reproducible and is not offered)."""

    def __init__(self, dev: Device, srs: Srs, max_degree: int, tau: int = None, g=None,
                 g2_points=None):
        self.dev = dev
        self.srs = srs
        self._max_degree = max_degree
        self._tau, self._g = tau, g
        self._shards = {}
        self._bytes = None  # (buffer, compressed, check) of from_bytes on a sharded device
        # the verifier's part of the CRS (kzg.rs:14-22): g1, g2 = g2_points[0],
        # g2_points[1] = tau g2 (kzg.rs:52-53)
        self.g1 = g if g is not None else G1_GENERATOR
        if g2_points is None and tau is not None:
            g2 = g2_generator()
            g2_points = [g2, g2_mul(g2, tau)]
        self.g2_points = g2_points

    @classmethod
    def trusted_setup(cls, max_degree: int, tau: int, dev: Device = None, g=None):
        """With a communicator attached (dev.world > 1) the SRS is held as shards:
        a polynomial of global length L is split over the ranks (rank r owns
        entries [r L/world, (r+1) L/world)) and each rank keeps the matching
        slice [tau^(r L/world + i)] g of the bases, generated on first use per L."""
        dev = dev or Device(0)
        if dev.world > 1:
            return cls(dev, None, max_degree, tau, g)
        return cls(dev, Srs.generate(dev, tau, max_degree + 1, g), max_degree, tau, g)

    def srs_for(self, n_local: int) -> Srs:
        """the bases a local vector of n_local entries is committed against"""
        if self.dev.world == 1:
            return self.srs
        if self.srs is not None and len(self.srs) == n_local:
            return self.srs  # a caller-provided shard of this length
        L = n_local * self.dev.world
        if L > self._max_degree + 1:
            raise QuillGpuError(-1, "Polynomial degree exceeds max degree")
        if self._tau is None and self._bytes is not None:
            if n_local not in self._shards:
                # an imported SRS: this rank's range of the bytes, validated on the
                # device, then (check=True) the powers check over all ranks' shards
                data, compressed, chk = self._bytes
                s = Srs.from_bytes(self.dev, data, compressed, offset=self.dev.rank * n_local,
                                   n=n_local)
                if chk and not s.check_powers(self.g1, self.g2_points):
                    s.close()
                    raise QuillGpuError(-5, "SRS powers check failed: the points are not "
                                            "[tau^i] g1 for the tau of g2_points")
                self._shards[n_local] = s
            return self._shards[n_local]
        if self._tau is None:
            raise QuillGpuError(-4, "sharded commitments need a generated (tau) SRS")
        if n_local not in self._shards:
            self._shards[n_local] = Srs.generate(self.dev, self._tau, n_local, self._g,
                                                 offset=self.dev.rank * n_local)
        return self._shards[n_local]

    def close(self):
        for s in [self.srs] + list(self._shards.values()):
            if s is not None:
                s.close()
        self._shards = {}

    @classmethod
    def from_points(cls, g1_points, dev: Device = None, g2_points=None):
        """an uploaded CRS; verification needs g2_points = [g2, tau g2] and
        takes g1 = g1_points[0]"""
        dev = dev or Device(0)
        return cls(dev, Srs.upload(dev, g1_points), len(g1_points) - 1, None, g1_points[0],
                   g2_points)

    @classmethod
    def from_bytes(cls, g1_bytes, g2_points, dev: Device = None, compressed: bool = True,
                   check: bool = True):
        """a CRS from ark-serialize G1 bytes (an ark `Vec` length prefix is
        stripped when present) and g2_points = [g2, tau g2]; g1 = the first
        point.  Every point is validated on the device (Srs.from_bytes);
        check=True also runs the powers check against g2_points and raises
        when it fails.  On a sharded device the buffer is kept (any buffer, e.g.
        an np.memmap) and srs_for(n_local) imports and checks this rank's range
        [rank n_local, (rank + 1) n_local) on first use."""
        dev = dev or Device(0)
        pb = 32 if compressed else 64
        arr = g1_bytes if isinstance(g1_bytes, np.ndarray) else np.frombuffer(g1_bytes,
                                                                              dtype=np.uint8)
        arr = arr.reshape(-1).view(np.uint8)
        if arr.size % pb == 8 and int.from_bytes(bytes(arr[:8]), "little") * pb == arr.size - 8:
            arr = arr[8:]
        if arr.size == 0 or arr.size % pb:
            raise QuillGpuError(-1, f"SRS bytes are not a positive multiple of {pb}")
        n = arr.size // pb
        one = Srs.from_bytes(dev, arr, compressed, offset=0, n=1)  # g1 = P_0, validated
        g1 = one.download()[0]
        one.close()
        if g1 is None:
            raise QuillGpuError(-1, "the first SRS point is the identity")
        if dev.world > 1:
            kzg = cls(dev, None, n - 1, None, g1, g2_points)
            kzg._bytes = (arr, compressed, check)
            return kzg
        srs = Srs.from_bytes(dev, arr, compressed)
        if check and not srs.check_powers(g1, g2_points):
            srs.close()
            raise QuillGpuError(-5, "SRS powers check failed: the points are not [tau^i] g1 "
                                    "for the tau of g2_points")
        return cls(dev, srs, n - 1, None, g1, g2_points)

    @classmethod
    def verifier(cls, tau: int = None, g1=None, g2_points=None):
        """the verifier's view only (g1, g2_points; no device SRS): built from
        tau like trusted_setup, or from published points"""
        if tau is None and g2_points is None:
            raise QuillGpuError(-1, "verifier needs tau or g2_points")
        return cls(None, None, -1, tau, g1, g2_points)

    def _vk(self) -> KzgVk:
        if self.g2_points is None:
            raise QuillGpuError(-1, "no G2 points: verification needs g2 and tau g2")
        vk = KzgVk()
        xy, inf = g1_to_abi(self.g1)
        if inf:
            raise QuillGpuError(-1, "g1 generator is the identity")
        C.memmove(vk.g1_xy, xy, 64)
        for fld, Q in (("g2_xy", self.g2_points[0]), ("g2_tau_xy", self.g2_points[1])):
            qxy, qinf = g2_to_abi(Q)
            if qinf:
                raise QuillGpuError(-1, "G2 point is the identity")
            C.memmove(getattr(vk, fld), qxy, 128)
        return vk

    def deferring(self, dev: Device = None, seed: bytes = None) -> "DeferringKZG":
        """a view of this key that collects pairing checks instead of running
        them (DeferringKZG): pass it wherever a verifier takes `pcs`, then call
        its check().  dev: fold the claims on that Device (qg_kzg_verify_batch_dev)
        instead of on the host; seed: 32 bytes of the verifier's own randomness
        mixed into the weights."""
        return DeferringKZG(self, dev, seed)

    # KZG::verify (kzg.rs:98-108)
    def verify_univariate(self, commitment, opening: KZGOpeningProof) -> bool:
        xy, inf = g1_to_abi(commitment)
        ok = C.c_int()
        check(lib().qg_kzg_verify(C.byref(self._vk()), xy, inf, C.byref(_opening_c(opening)),
                                  C.byref(ok)))
        return bool(ok.value)

    def folding(self) -> "FoldingKZG":
        """a view of this key whose open, open_dev and open_batch_dev return
        folded openings (FoldingKZG): pass it wherever a prover takes `pcs`.
        Single-context only."""
        return FoldingKZG(self)

    # MultilinearPCS::verify == MLEvalProof::verify (lib.rs:35-40, mlpcs.rs:126-161);
    # a FoldedMLEvalProof goes to the folded verifier
    def verify(self, commitment, proof, transcript: Transcript) -> bool:
        xy, inf = g1_to_abi(commitment)
        pt = proof.evaluation_point
        arr = fr_array(pt) if len(pt) else np.zeros((1, 4), dtype=np.uint64)
        ok = C.c_int()
        if isinstance(proof, FoldedMLEvalProof):
            check(lib().qg_mle_verify_folded(C.byref(self._vk()), xy, inf, u64p(arr), len(pt),
                                             C.byref(_folded_proof_c(proof)),
                                             transcript.c_state(), C.byref(ok)))
            return bool(ok.value)
        check(lib().qg_mle_verify(C.byref(self._vk()), xy, inf, u64p(arr), len(pt),
                                  C.byref(_mle_proof_c(proof)), transcript.c_state(),
                                  C.byref(ok)))
        return bool(ok.value)

    # MultilinearPCS::max_degree (lib.rs:32)
    def max_degree(self) -> int:
        return self._max_degree

    # KZG::commit (kzg.rs:61-73) == MultilinearPCS::commit (mlpcs.rs:187-189)
    def commit(self, poly):
        if len(poly) > self._max_degree + 1:
            raise QuillGpuError(-1, "Polynomial degree exceeds max degree")
        if isinstance(poly, DeviceVec):
            return self.srs_for(len(poly)).msm_dev(poly, len(poly))
        arr = fr_array(poly) if len(poly) else np.zeros((1, 4), dtype=np.uint64)
        xy = (C.c_uint64 * 8)()
        inf = C.c_uint8()
        check(lib().qg_kzg_commit(self.dev.h, self.srs.h, u64p(arr), len(poly), xy,
                                  C.byref(inf)), self.dev.h)
        return g1_from_abi(xy, inf.value)

    def commit_batch(self, polys) -> list:
        """[commit(p) for p in polys], device vectors of one SRS shard as one MSM
        batch (qg_msm_g1_dev_batch); the same points"""
        if (len(polys) < 2 or not all(isinstance(p, DeviceVec) for p in polys)
                or (self.dev.world > 1 and len({len(p) for p in polys}) != 1)
                or os.environ.get("QUILL_COMMIT_BATCH", "1") == "0"):  # A/B runs
            return [self.commit(p) for p in polys]
        for p in polys:
            if len(p) > self._max_degree + 1:
                raise QuillGpuError(-1, "Polynomial degree exceeds max degree")
        return self.srs_for(len(polys[0])).msm_dev_batch(polys)

    # KZG::open (kzg.rs:75-96)
    def open_univariate(self, poly, x: int) -> KZGOpeningProof:
        arr = fr_array(poly) if len(poly) else np.zeros((1, 4), dtype=np.uint64)
        out = KzgOpening()
        check(lib().qg_kzg_open(self.dev.h, self.srs.h, u64p(arr), len(poly), fr_c(x),
                                C.byref(out)), self.dev.h)
        return _opening(out)

    def open_lincomb_dev(self, vecs, lens, coeffs, xs) -> list:
        """KZG::open of sum_j coeffs[j] vecs[j][:lens[j]] at the one or two
        points xs, the combination formed inside the quotient scan
        (qg_kzg_open_lincomb_dev; the folded opening's building block)"""
        P, nx = len(vecs), len(xs)
        hs = (C.c_void_p * max(P, 1))(*[v.h.value for v in vecs])
        ls = (C.c_size_t * max(P, 1))(*lens)
        cs = fr_array(coeffs) if P else np.zeros((1, 4), dtype=np.uint64)
        xa = fr_array(xs) if nx else np.zeros((1, 4), dtype=np.uint64)
        outs = (KzgOpening * max(nx, 1))()
        check(lib().qg_kzg_open_lincomb_dev(self.dev.h, self.srs.h if self.srs else None, hs, ls,
                                            u64p(cs), P, u64p(xa), nx, outs), self.dev.h)
        return [_opening(outs[i]) for i in range(nx)]

    # MultilinearPCS::open == MLEvalProof::prove (mlpcs.rs:83-124, 191-198)
    def open_dev(self, vec, n, eval_point, transcript: Transcript,
                 unchanged: bool = False) -> MLEvalProof:
        """open() on the first n entries of a device-resident DeviceVec.
        unchanged=True: vec has not changed since an earlier open of it on this
        device (qg_mle_open_dev_ex QG_OPEN_UNCHANGED: its transform is reused)"""
        pt = fr_array(eval_point) if len(eval_point) else np.zeros((1, 4), dtype=np.uint64)
        out = MleProof()
        check(lib().qg_mle_open_dev_ex(self.dev.h, self.srs_for(n).h, vec.h, n, u64p(pt),
                                       len(eval_point), transcript.c_state(),
                                       1 if unchanged else 0, C.byref(out)), self.dev.h)
        return MLEvalProof(list(eval_point), fr_from_mont_limbs(list(out.evaluation)),
                           g1_from_abi(out.s_comm_xy, out.s_comm_inf),
                           _opening(out.poly_opening), _opening(out.poly_opening_inv),
                           _opening(out.s_opening), _opening(out.s_opening_inv))

    def open_batch_dev(self, items, transcript: Transcript) -> list:
        """K openings [(vec, n, eval_point, unchanged), ...] in one call
        (qg_mle_open_batch_dev): the same proofs and transcript as K successive
        open_dev calls, with the S and quotient commitments as two MSM batches.
        Sharded devices batch each run of consecutive items of one local length
        (they commit against one SRS shard; mle_open_batch_sharded): the runs
        keep the item order, so the transcript is the same."""
        if len(items) <= 1:
            return [self.open_dev(v, n, pt, transcript, unch) for v, n, pt, unch in items]
        if self.dev.world > 1:
            out, i = [], 0
            while i < len(items):
                j = i
                while j < len(items) and items[j][1] == items[i][1]:
                    j += 1
                out += self._open_batch(items[i:j], transcript, self.srs_for(items[i][1]))
                i = j
            return out
        return self._open_batch(items, transcript, self.srs)

    def _open_batch(self, items, transcript: Transcript, srs) -> list:
        if len(items) == 1:
            v, n, pt, unch = items[0]
            return [self.open_dev(v, n, pt, transcript, unch)]
        k = len(items)
        arr = (MleOpenItem * k)()
        pts = []
        for i, (vec, n, pt, unch) in enumerate(items):
            a = fr_array(pt) if len(pt) else np.zeros((1, 4), dtype=np.uint64)
            pts.append(a)  # kept alive through the call
            arr[i] = MleOpenItem(vec.h.value, n, a.ctypes.data_as(C.POINTER(C.c_uint64)), len(pt),
                                 1 if unch else 0, 0)
        outs = (MleProof * k)()
        check(lib().qg_mle_open_batch_dev(self.dev.h, srs.h, arr, k, transcript.c_state(),
                                          outs), self.dev.h)
        return [MLEvalProof(list(pt), fr_from_mont_limbs(list(o.evaluation)),
                            g1_from_abi(o.s_comm_xy, o.s_comm_inf),
                            _opening(o.poly_opening), _opening(o.poly_opening_inv),
                            _opening(o.s_opening), _opening(o.s_opening_inv))
                for (_, _, pt, _), o in zip(items, outs)]

    def open_multi(self, polys, claims, transcript: Transcript):
        """k evaluation claims [(j, point), ...] over the device vectors `polys`
        as one sumcheck and one opening (MultiOpenProof.prove, multiopen.py)"""
        from .multiopen import MultiOpenProof
        return MultiOpenProof.prove(polys, claims, self, transcript)

    def open(self, poly, eval_point, transcript: Transcript,
             unchanged: bool = False) -> MLEvalProof:
        if isinstance(poly, DeviceVec):
            return self.open_dev(poly, len(poly), eval_point, transcript, unchanged)
        arr = fr_array(poly) if len(poly) else np.zeros((1, 4), dtype=np.uint64)
        pt = fr_array(eval_point) if len(eval_point) else np.zeros((1, 4), dtype=np.uint64)
        out = MleProof()
        check(lib().qg_mle_open(self.dev.h, self.srs.h, u64p(arr), len(poly), u64p(pt),
                                len(eval_point), transcript.c_state(), C.byref(out)), self.dev.h)
        return MLEvalProof(list(eval_point), fr_from_mont_limbs(list(out.evaluation)),
                           g1_from_abi(out.s_comm_xy, out.s_comm_inf),
                           _opening(out.poly_opening), _opening(out.poly_opening_inv),
                           _opening(out.s_opening), _opening(out.s_opening_inv))


class FoldingKZG:
    """The folded ML opening as a view of a KZG key (KZG.folding()): open,
    open_dev and open_batch_dev return FoldedMLEvalProofs (qg_mle_open_folded_dev
    / _batch_dev: 3 MSMs and 2 KZG claims per opening instead of 5 and 4); every
    other attribute is the key's.  KZG.verify and DeferringKZG.verify take the
    proofs as they take MLEvalProofs."""

    def __init__(self, base: "KZG"):
        if base.dev is not None and (base.dev.world > 1 or base.dev.comm_info()["sharded"]):
            raise ValueError("the folded opening is not supported on a sharded device "
                             "(communicator attached)")
        self.base = base

    def __getattr__(self, name):
        return getattr(self.base, name)

    def folding(self) -> "FoldingKZG":
        return self

    def open_dev(self, vec, n, eval_point, transcript: Transcript,
                 unchanged: bool = False) -> FoldedMLEvalProof:
        pt = fr_array(eval_point) if len(eval_point) else np.zeros((1, 4), dtype=np.uint64)
        out = MleProofFolded()
        dev = self.base.dev
        check(lib().qg_mle_open_folded_dev(dev.h, self.base.srs_for(n).h, vec.h, n, u64p(pt),
                                           len(eval_point), transcript.c_state(),
                                           1 if unchanged else 0, C.byref(out)), dev.h)
        return _folded_proof(eval_point, out)

    def open_batch_dev(self, items, transcript: Transcript) -> list:
        """K folded openings [(vec, n, eval_point, unchanged), ...] in one call:
        the same proofs and transcript as K successive open_dev calls"""
        if len(items) <= 1:
            return [self.open_dev(v, n, pt, transcript, unch) for v, n, pt, unch in items]
        k = len(items)
        arr = (MleOpenItem * k)()
        pts = []
        for i, (vec, n, pt, unch) in enumerate(items):
            a = fr_array(pt) if len(pt) else np.zeros((1, 4), dtype=np.uint64)
            pts.append(a)  # kept alive through the call
            arr[i] = MleOpenItem(vec.h.value, n, a.ctypes.data_as(C.POINTER(C.c_uint64)), len(pt),
                                 1 if unch else 0, 0)
        outs = (MleProofFolded * k)()
        dev = self.base.dev
        check(lib().qg_mle_open_folded_batch_dev(dev.h, self.base.srs.h, arr, k,
                                                 transcript.c_state(), outs), dev.h)
        return [_folded_proof(pt, o) for (_, _, pt, _), o in zip(items, outs)]

    def open_multi(self, polys, claims, transcript: Transcript):
        from .multiopen import MultiOpenProof
        return MultiOpenProof.prove(polys, claims, self, transcript)

    def open(self, poly, eval_point, transcript: Transcript,
             unchanged: bool = False) -> FoldedMLEvalProof:
        if isinstance(poly, DeviceVec):
            return self.open_dev(poly, len(poly), eval_point, transcript, unchanged)
        vec = DeviceVec.from_list(self.base.dev, list(poly) if len(poly) else [0])
        try:
            return self.open_dev(vec, len(poly), eval_point, transcript)
        finally:
            vec.close()


_MLE_OPENINGS = ("poly_opening", "poly_opening_inv", "s_opening", "s_opening_inv")


def _claim_c(commitment, opening: KZGOpeningProof) -> KzgClaim:
    c = KzgClaim()
    xy, inf = g1_to_abi(commitment)
    C.memmove(c.comm_xy, xy, 64)
    c.comm_inf = inf
    c.opening = _opening_c(opening)
    return c


def _claim_copy(c: KzgClaim) -> KzgClaim:
    out = KzgClaim()
    C.memmove(C.byref(out), C.byref(c), C.sizeof(KzgClaim))
    return out


class DeferringKZG:
    """Batched verification (qg_kzg_verify_batch): a view of a KZG key whose
    verify, verify_univariate and InnerProductProof.verify path run everything
    but the pairing checks, append those as claims and return only the
    non-pairing verdict (the ML / inner-product equation; True for a univariate
    opening).  check() then verifies every collected claim with ONE pairing
    check - two Miller loops and one final exponentiation, the fold on the host
    or, with `dev`, as two device MSMs.  Every other attribute is the key's.

    `claims` holds (label, KzgClaim) in call order.  A label is `labels[id(proof)]`
    when the caller registered the proof object there, else "opening <k>" for
    the k-th deferred call; the opening's field name is appended.  `messages`
    maps id(proof) to the error text check() raises for that proof's claims.

    Accepted set: what the sequential verifier accepts is accepted; a set with
    a false opening is accepted with probability at most about 2^-128 (the
    weights are 128-bit Fiat-Shamir values over all the claims)."""

    def __init__(self, base: "KZG", dev: Device = None, seed: bytes = None):
        if seed is not None and len(seed) != 32:
            raise QuillGpuError(-1, "the batch seed is 32 bytes")
        self.base, self.batch_dev, self.seed = base, dev, seed
        self.claims, self.labels, self.messages = [], {}, {}
        self._msgs = []
        self._calls = 0

    def __getattr__(self, name):
        return getattr(self.base, name)

    def _push(self, proof, names, cs):
        label = self.labels.get(id(proof), f"opening {self._calls}")
        self._calls += 1
        for name, c in zip(names, cs):
            self.claims.append((f"{label}, {name}" if name else label, _claim_copy(c)))
            self._msgs.append(self.messages.get(id(proof), "KZG opening verification failed"))

    def verify_univariate(self, commitment, opening: KZGOpeningProof) -> bool:
        self._push(opening, (None,), (_claim_c(commitment, opening),))
        return True

    def verify(self, commitment, proof, transcript: Transcript) -> bool:
        xy, inf = g1_to_abi(commitment)
        pt = proof.evaluation_point
        arr = fr_array(pt) if len(pt) else np.zeros((1, 4), dtype=np.uint64)
        if isinstance(proof, FoldedMLEvalProof):
            ok, out = C.c_int(), (KzgClaim * 2)()
            check(lib().qg_mle_verify_folded_defer(C.byref(self.base._vk()), xy, inf, u64p(arr),
                                                   len(pt), C.byref(_folded_proof_c(proof)),
                                                   transcript.c_state(), out, C.byref(ok)))
            self._push(proof, _FOLDED_CLAIMS, out)
            return bool(ok.value)
        ok, out = C.c_int(), (KzgClaim * 4)()
        check(lib().qg_mle_verify_defer(C.byref(self.base._vk()), xy, inf, u64p(arr), len(pt),
                                        C.byref(_mle_proof_c(proof)), transcript.c_state(), out,
                                        C.byref(ok)))
        self._push(proof, _MLE_OPENINGS, out)
        return bool(ok.value)

    def verify_inner_product(self, comm1, comm2, proof, transcript: Transcript) -> bool:
        xy1, inf1 = g1_to_abi(comm1)
        xy2, inf2 = g1_to_abi(comm2)
        if isinstance(proof, FoldedInnerProductProof):
            ok, out = C.c_int(), (KzgClaim * 2)()
            check(lib().qg_ipa_verify_folded_defer(C.byref(self.base._vk()), xy1, inf1, xy2, inf2,
                                                   C.byref(_ipa_folded_proof_c(proof)),
                                                   transcript.c_state(), out, C.byref(ok)))
            self._push(proof, _FOLDED_CLAIMS, out)
            return bool(ok.value)
        ok, out = C.c_int(), (KzgClaim * 6)()
        check(lib().qg_ipa_verify_defer(C.byref(self.base._vk()), xy1, inf1, xy2, inf2,
                                        C.byref(_ipa_proof_c(proof)), transcript.c_state(), out,
                                        C.byref(ok)))
        self._push(proof, _IPA_OPENINGS, out)
        return bool(ok.value)

    def check(self) -> None:
        """one pairing check over every claim collected so far.  Raises
        ValueError naming the label of the lowest failing claim (found by a
        sequential scan that only a rejection pays for); the claims stay."""
        n = len(self.claims)
        arr = (KzgClaim * max(n, 1))()
        for i, (_, c) in enumerate(self.claims):
            arr[i] = c
        seed = None if self.seed is None else (C.c_uint8 * 32).from_buffer_copy(self.seed)
        ok, bad = C.c_int(), C.c_size_t()
        vk = self.base._vk()
        if self.batch_dev is not None:
            check(lib().qg_kzg_verify_batch_dev(self.batch_dev.h, C.byref(vk), arr, n, seed,
                                                C.byref(ok), C.byref(bad)), self.batch_dev.h)
        else:
            check(lib().qg_kzg_verify_batch(C.byref(vk), arr, n, seed, C.byref(ok),
                                            C.byref(bad)))
        if not ok.value:
            raise ValueError(f"{self._msgs[bad.value]} ({self.claims[bad.value][0]}; "
                             f"batched claim {bad.value} of {n})")
