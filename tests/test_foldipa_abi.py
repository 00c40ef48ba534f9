"""The folded inner-product argument's C ABI on the CPU: the entries are
declared in the header, bound in PROTOTYPES, exported and listed in
INTEGRATION.md; null handles are QG_ERR_INVALID; the ctypes struct has the
header's layout."""
import ctypes as C
import os
import re

INVALID = -1
ENTRIES = ("qg_ipa_prove_folded", "qg_ipa_prove_folded_dev", "qg_ipa_verify_folded",
           "qg_ipa_verify_folded_defer", "qg_poly_eval2_dev")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "quill_gpu.h")).read()


def test_entries_declared_bound_and_exported():
    import quill_amd
    from quill_amd._lib import PROTOTYPES
    txt, L = _header(), quill_amd.lib()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in PROTOTYPES and hasattr(L, name), name
        assert re.search(r"\bint %s\s*\(" % name, txt), name
        assert re.search(r"\bfn %s\s*\(" % name, integ), name
    for name in ("FoldedInnerProductProof",):
        assert hasattr(quill_amd, name)
    assert hasattr(quill_amd.Device, "poly_eval2")


def test_struct_layout_matches_the_header():
    from quill_amd._lib import IpaProofFolded
    m = re.search(r"typedef struct qg_ipa_proof_folded \{([^}]*)\} qg_ipa_proof_folded;", _header())
    assert m
    # the header's members in order: name, element type, element count
    size = {"uint64_t": 8, "uint8_t": 1}
    off = 0
    for ty, name, dims in re.findall(r"(uint64_t|uint8_t)\s+(\w+)((?:\[\d+\])*)\s*;", m.group(1)):
        n = 1
        for d in re.findall(r"\[(\d+)\]", dims):
            n *= int(d)
        assert off % size[ty] == 0
        f = getattr(IpaProofFolded, name)
        assert (f.offset, f.size) == (off, n * size[ty]), name
        off += n * size[ty]
    assert off == C.sizeof(IpaProofFolded) == 32 + 72 + 192 + 72 + 72
    assert IpaProofFolded.y.offset == 104 and IpaProofFolded.w_xy.offset == 296


def test_null_handles_are_invalid():
    import quill_amd
    from quill_amd._lib import IpaProofFolded, KzgVk
    L = quill_amd.lib()
    ok = C.c_int()
    assert L.qg_ipa_prove_folded(None, None, None, 0, None, 0, None, None) == INVALID
    assert L.qg_ipa_prove_folded_dev(None, None, None, 0, None, 0, None, None) == INVALID
    assert L.qg_poly_eval2_dev(None, None, None, 1, None, None) == INVALID
    assert L.qg_ipa_verify_folded(None, None, 0, None, 0, None, None, C.byref(ok)) == INVALID
    assert L.qg_ipa_verify_folded_defer(None, None, 0, None, 0, None, None, None,
                                        C.byref(ok)) == INVALID
    # a proof without a key, a key without a proof, no place for the claims
    st = (C.c_uint8 * 32)()
    xy = (C.c_uint64 * 8)()
    proof = IpaProofFolded()
    assert L.qg_ipa_verify_folded(None, xy, 1, xy, 1, C.byref(proof), st, C.byref(ok)) == INVALID
    assert L.qg_ipa_verify_folded(C.byref(KzgVk()), xy, 1, xy, 1, None, st,
                                  C.byref(ok)) == INVALID
    assert L.qg_ipa_verify_folded_defer(C.byref(KzgVk()), xy, 1, xy, 1, C.byref(proof), st, None,
                                        C.byref(ok)) == INVALID
    assert bytes(st) == bytes(32)
