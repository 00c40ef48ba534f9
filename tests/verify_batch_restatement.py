"""The batched KZG check (qg_kzg_verify_batch) restated on the oracle's
primitives, for the CPU and GPU tests of the fold.

A claim is (C, x, y, pi): a commitment, and an opening of it at x to y with the
quotient commitment pi.  The weights come from a transcript of their own
(include/quill_gpu.h, qg_kzg_batch_fold): domain "quill_kzg_batch", n as a u64,
per claim C, x, y, pi, then the optional 32 seed bytes; rho_0 = 1 and rho_i =
the i-th drawn field element mod 2^128."""
import ctypes as C

import pairing_oracle as po
import quill_oracle as o

R = o.R_MOD


def weights(claims, seed=None):
    t = o.Transcript(b"quill_kzg_batch")
    t.append_u64(len(claims))
    for Cm, x, y, pi in claims:
        t.append_g1(Cm)
        t.append_fr(x)
        t.append_fr(y)
        t.append_g1(pi)
    if seed is not None:
        t.append_bytes(seed)
    return [1] + [t.draw_field_element() % (1 << 128) for _ in range(len(claims) - 1)]


def fold(claims, seed=None, g1=po.G1_GEN, rho=None):
    """(L, R) = (sum rho_i (C_i - y_i g1 + x_i pi_i), sum rho_i pi_i)"""
    rho = weights(claims, seed) if rho is None else rho
    L = Rr = None
    ysum = 0
    for r, (Cm, x, y, pi) in zip(rho, claims):
        L = po.g1_add(L, po.g1_mul(Cm, r))
        L = po.g1_add(L, po.g1_mul(pi, r * x % R))
        Rr = po.g1_add(Rr, po.g1_mul(pi, r))
        ysum = (ysum + r * y) % R
    L = po.g1_add(L, po.g1_mul(g1, (R - ysum) % R))
    return L, Rr


def trapdoor_claim(tau, c, x, y=None):
    """a valid claim of the constant-free family C = c g1 opened at x to y:
    pi = ((c - y) / (tau - x)) g1.  y = None picks y = c - (tau - x) (pi = g1)."""
    if y is None:
        y = (c - (tau - x)) % R
    k = (c - y) * pow((tau - x) % R, R - 2, R) % R
    return (po.g1_mul(po.G1_GEN, c), x % R, y % R, po.g1_mul(po.G1_GEN, k))


def claims_c(q, claims):
    from quill_amd._lib import KzgClaim
    from quill_amd.pcs import _claim_c
    arr = (KzgClaim * max(len(claims), 1))()
    for i, (Cm, x, y, pi) in enumerate(claims):
        arr[i] = _claim_c(Cm, q.KZGOpeningProof(x, y, pi))
    return arr


def claim_py(c):
    """KzgClaim -> (C, x, y, pi)"""
    from quill_amd.field import fr_from_mont_limbs, g1_from_abi
    op = c.opening
    return (g1_from_abi(c.comm_xy, c.comm_inf), fr_from_mont_limbs(list(op.x)),
            fr_from_mont_limbs(list(op.y)), g1_from_abi(op.proof_xy, op.proof_inf))


def _seed_c(seed):
    return None if seed is None else (C.c_uint8 * 32).from_buffer_copy(seed)


def call_fold(q, vk, claims, seed=None, dev=None):
    """(rc, L, R) from qg_kzg_batch_fold, or _dev on `dev`"""
    from quill_amd.field import g1_from_abi
    L = q.lib()
    lxy, rxy = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
    linf, rinf = C.c_uint8(), C.c_uint8()
    arr = claims_c(q, claims)
    k = vk._vk()
    if dev is None:
        rc = L.qg_kzg_batch_fold(C.byref(k), arr, len(claims), _seed_c(seed), lxy, C.byref(linf),
                                 rxy, C.byref(rinf))
    else:
        rc = L.qg_kzg_batch_fold_dev(dev.h, C.byref(k), arr, len(claims), _seed_c(seed), lxy,
                                     C.byref(linf), rxy, C.byref(rinf))
    if rc:
        return rc, None, None
    return rc, g1_from_abi(lxy, linf.value), g1_from_abi(rxy, rinf.value)


UNTOUCHED = 0xDEAD


def call_verify(q, vk, claims, seed=None, dev=None):
    """(rc, ok, first_bad) from qg_kzg_verify_batch, or _dev on `dev`;
    first_bad is UNTOUCHED when the call did not write it"""
    L = q.lib()
    ok, bad = C.c_int(-1), C.c_size_t(UNTOUCHED)
    arr = claims_c(q, claims)
    k = vk._vk()
    if dev is None:
        rc = L.qg_kzg_verify_batch(C.byref(k), arr, len(claims), _seed_c(seed), C.byref(ok),
                                   C.byref(bad))
    else:
        rc = L.qg_kzg_verify_batch_dev(dev.h, C.byref(k), arr, len(claims), _seed_c(seed),
                                       C.byref(ok), C.byref(bad))
    return rc, ok.value, bad.value
