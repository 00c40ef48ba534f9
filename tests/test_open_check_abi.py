"""The opening check's C-ABI additions, without a GPU: qg_poly_eval_dev and the
test-only qg_debug_open_fault are declared in include/quill_gpu.h, bound in
quill_amd._lib.PROTOTYPES and exported by the library, and they (like
qg_ctx_counter) reject null handles with QG_ERR_INVALID before touching a
device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "quill_gpu.h")
NEW = ("qg_poly_eval_dev", "qg_debug_open_fault")


@pytest.fixture(scope="module")
def L():
    from quill_amd import lib
    return lib()


@pytest.mark.parametrize("name", NEW)
def test_declared_bound_and_exported(L, name):
    from quill_amd._lib import PROTOTYPES
    txt = open(HEADER).read()
    assert re.search(r"\bint\s+%s\s*\(" % name, txt), "not in the header"
    assert name in PROTOTYPES
    assert hasattr(L, name)


def test_header_documents_the_fault_hook_as_test_only():
    txt = open(HEADER).read()
    doc = txt[:txt.index("int qg_debug_open_fault")]
    assert "TEST ONLY" in doc[doc.rindex("/*"):]


def test_null_handles_are_invalid(L):
    x = (C.c_uint64 * 4)(1, 0, 0, 0)
    out = (C.c_uint64 * 4)()
    assert L.qg_poly_eval_dev(None, None, 0, x, 0, out) == -1
    assert L.qg_debug_open_fault(None, 1, 0) == -1
    v = C.c_uint64()
    assert L.qg_ctx_counter(None, b"open_checks", C.byref(v)) == -1
    assert L.qg_ctx_counter(None, b"open_check_failures", C.byref(v)) == -1
