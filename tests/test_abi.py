"""C-ABI checks that need no GPU: the shared library loads, exports every
entry point include/quill_gpu.h declares, and its host-side pieces (BLAKE3
transcript, ark-serialize encodings, expression degree, argument validation)
agree with the oracle byte for byte."""
import ctypes as C
import os
import random
import re

import pytest

import quill_oracle as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "quill_gpu.h")


def header_symbols():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(qg_[a-z0-9_]+)\s*\(", txt)))


@pytest.fixture(scope="module")
def L():
    from quill_amd import lib
    return lib()


def test_library_exports_every_declared_symbol(L):
    syms = header_symbols()
    assert len(syms) >= 30
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, missing


def test_python_prototypes_cover_header():
    from quill_amd._lib import PROTOTYPES
    assert set(header_symbols()) == set(PROTOTYPES)


def test_version(L):
    assert b"gfx950" in L.qg_version()


def test_transcript_parity_with_oracle():
    from quill_amd import Transcript
    rnd = random.Random(1)
    for dom in (b"", b"sumcheck_bench", bytes(range(256)) * 9):
        a, b = Transcript(dom), o.Transcript(dom)
        assert a.state == b.state
        for _ in range(10):
            m = bytes(rnd.randrange(256) for _ in range(rnd.choice([0, 31, 64, 1000, 1024, 2100])))
            a.append_bytes(m)
            b.append_bytes(m)
            x = rnd.randrange(o.R_MOD)
            a.append_fr(x)
            b.append_fr(x)
            a.append_fr_vec([x, 1, 2])
            b.append_fr_vec([x, 1, 2])
            a.append_poly([x, 0, 0])
            b.append_poly([x, 0, 0])
            a.append_u64(77)
            b.append_u64(77)
            assert a.state == b.state
            assert a.draw_field_element() == b.draw_field_element()
            assert a.draw_challenge(64) == b.draw_challenge(64)


def test_draw_field_element_fuzz_vs_oracle():
    """from_le_bytes_mod_order of the 48 XOF bytes (transcript.rs:70-74) for
    random states: the low 256 bits exceed r for ~80 % of draws and must be
    reduced before the Montgomery conversion (a lost top carry once made ~2 %
    of challenges wrong)."""
    from quill_amd import Transcript
    rnd = random.Random(7)
    for _ in range(3000):
        st = bytes(rnd.randrange(256) for _ in range(32))
        a, b = Transcript(b""), o.Transcript(b"")
        a.state = st
        b.state = st
        assert a.draw_field_element() == b.draw_field_element()


def test_g1_serialize_parity_with_oracle():
    from quill_amd import Transcript
    rnd = random.Random(2)
    pts = [None, o.G1_GEN, o.g1_neg(o.G1_GEN)] + [o.g1_mul(o.G1_GEN, rnd.randrange(o.R_MOD))
                                                  for _ in range(20)]
    for P in pts:
        a, b = Transcript(b"g"), o.Transcript(b"g")
        a.append_g1(P)
        b.append_g1(P)
        assert a.state == b.state


def test_expr_degree():
    from quill_amd.hyperplonk import VirtualPolyExpr as E, expr_degree
    assert expr_degree(E.Input(0) * E.Input(1) * E.Input(2)) == 3
    assert expr_degree(E.Input(0) * E.Input(0) - E.Input(1)) == 2
    assert expr_degree(E.Const(5) + E.Input(1)) == 1
    assert expr_degree(E.Const(5)) == 0


def test_invalid_arguments_return_status(L):
    from quill_amd._lib import ExprOp
    # malformed program (stack underflow) -> QG_ERR_INVALID, no crash
    prog = (ExprOp * 1)(ExprOp(2, 0))
    d = C.c_uint32()
    assert L.qg_expr_degree(prog, 1, C.byref(d)) == -1
    assert L.qg_transcript_draw(None, None, 0) == -1
    st = (C.c_uint8 * 32)()
    out = (C.c_uint8 * 65)()
    assert L.qg_transcript_draw(st, out, 65) == -1  # > 64 bytes
    assert L.qg_ctx_create(0, None) == -1
    # round-6 entry points: null handles / callbacks are rejected before any
    # device work (QG_ERR_INVALID)
    h = C.c_void_p()
    xy = (C.c_uint64 * 8)()
    inf = C.c_uint8()
    assert L.qg_bases_upload(None, xy, None, 1, C.byref(h)) == -1
    assert L.qg_msm_g1_at(None, None, 0, None, 0, xy, C.byref(inf)) == -1
    assert L.qg_msm_g1_dev_at(None, None, 0, None, 0, xy, C.byref(inf)) == -1
    assert L.qg_msm_g1_dev_batch(None, None, None, None, 0, None, None) == -1
    assert L.qg_sumcheck_prove_cb(None, 1, 0, None, prog, 1, None, 0, C.cast(None, L.qg_sumcheck_prove_cb.argtypes[8]),
                                  None, None, None, None, None) == -1
    assert L.qg_ctx_phase_split(None, None, 0, None) == -1
    # the 29-bit-limb self-tests: null pointers, unknown op / field, too many
    # cases, a device run without a context -> QG_ERR_INVALID, never a fault
    w = (C.c_uint32 * 144)()
    fl = (C.c_uint32 * 1)()
    assert L.qg_selftest_field29(None, 1, 0, 0, None, 1, w) == -1
    assert L.qg_selftest_field29(None, 1, 0, 0, w, 1, None) == -1
    assert L.qg_selftest_field29(None, 2, 0, 0, w, 1, w) == -1
    assert L.qg_selftest_field29(None, -1, 0, 0, w, 1, w) == -1
    assert L.qg_selftest_field29(None, 1, 21, 0, w, 1, w) == -1
    assert L.qg_selftest_field29(None, 1, -1, 0, w, 1, w) == -1
    assert L.qg_selftest_field29(None, 1, 0, 0, w, 65537, w) == -1
    assert L.qg_selftest_field29(None, 1, 0, 1, w, 1, w) == -1
    assert L.qg_selftest_field29(None, 1, 0, 0, w, 1, w) == 0
    assert L.qg_selftest_curve29(None, 0, 0, None, 1, w, fl) == -1
    assert L.qg_selftest_curve29(None, 0, 0, w, 1, None, fl) == -1
    assert L.qg_selftest_curve29(None, 0, 0, w, 1, w, None) == -1
    assert L.qg_selftest_curve29(None, 8, 0, w, 1, w, fl) == -1
    assert L.qg_selftest_curve29(None, -1, 0, w, 1, w, fl) == -1
    assert L.qg_selftest_curve29(None, 0, 0, w, 65537, w, fl) == -1
    assert L.qg_selftest_curve29(None, 0, 1, w, 1, w, fl) == -1
    assert L.qg_selftest_curve29(None, 0, 0, w, 1, w, fl) == 0
    assert L.qg_selftest_msm_fold(None, 1, w, w, 1, 1, 1, 0, w, None) == -1


def test_no_device_is_an_error_not_a_fallback():
    """Without a HIP device the product refuses to run (no CPU path)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from quill_amd import Device, QuillGpuError
    with pytest.raises(QuillGpuError):
        Device(0)
