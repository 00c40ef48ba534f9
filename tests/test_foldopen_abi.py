"""The folded opening's C ABI on the CPU: the entries are declared in the
header, bound in PROTOTYPES and exported; null handles are QG_ERR_INVALID; the
ctypes struct has the header's layout."""
import ctypes as C
import os
import re

INVALID = -1
ENTRIES = ("qg_mle_open_folded_dev", "qg_mle_open_folded_batch_dev", "qg_mle_verify_folded",
           "qg_mle_verify_folded_defer", "qg_kzg_open_lincomb_dev")


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "quill_gpu.h")).read()


def test_entries_declared_bound_and_exported():
    import quill_amd
    from quill_amd._lib import PROTOTYPES
    txt, L = _header(), quill_amd.lib()
    integ = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                              "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in PROTOTYPES and hasattr(L, name), name
        assert re.search(r"\bint %s\s*\(" % name, txt), name
        assert re.search(r"\bfn %s\s*\(" % name, integ), name


def test_struct_layout_matches_the_header():
    from quill_amd._lib import MleProofFolded
    m = re.search(r"typedef struct qg_mle_proof_folded \{([^}]*)\} qg_mle_proof_folded;", _header())
    assert m
    # the header's members in order: name, element type, element count
    size = {"uint64_t": 8, "uint8_t": 1}
    off = 0
    for ty, name, dims in re.findall(r"(uint64_t|uint8_t)\s+(\w+)((?:\[\d+\])*)\s*;", m.group(1)):
        n = 1
        for d in re.findall(r"\[(\d+)\]", dims):
            n *= int(d)
        assert off % size[ty] == 0
        f = getattr(MleProofFolded, name)
        assert (f.offset, f.size) == (off, n * size[ty]), name
        off += n * size[ty]
    assert off == C.sizeof(MleProofFolded) == 32 + 72 + 128 + 72 + 72
    assert MleProofFolded.y.offset == 104 and MleProofFolded.w_xy.offset == 232


def test_null_handles_are_invalid():
    import quill_amd
    L = quill_amd.lib()
    ok = C.c_int()
    assert L.qg_mle_open_folded_dev(None, None, None, 0, None, 0, None, 0, None) == INVALID
    assert L.qg_mle_open_folded_batch_dev(None, None, None, 0, None, None) == INVALID
    assert L.qg_mle_verify_folded(None, None, 0, None, 0, None, None, C.byref(ok)) == INVALID
    assert L.qg_mle_verify_folded_defer(None, None, 0, None, 0, None, None, None,
                                        C.byref(ok)) == INVALID
    assert L.qg_kzg_open_lincomb_dev(None, None, None, None, None, 1, None, 1, None) == INVALID
    # a proof without a key, a key without a proof
    from quill_amd._lib import KzgVk, MleProofFolded
    st = (C.c_uint8 * 32)()
    xy = (C.c_uint64 * 8)()
    assert L.qg_mle_verify_folded(None, xy, 1, None, 0, C.byref(MleProofFolded()), st,
                                  C.byref(ok)) == INVALID
    assert L.qg_mle_verify_folded(C.byref(KzgVk()), xy, 1, None, 0, None, st,
                                  C.byref(ok)) == INVALID
