"""CPU unit test of the lookup multiplicities' host-side decisions
(csrc/lookup_plan.h), the part of the hash-partitioned sharded flow that is a
pure function of the world size, the lengths and the gathered record counts:
the owner of a tuple (below W for W = 1..8 and non-powers of two, rank 0 with
QG_LOOKUP_OWNER_BITS=0), the agreed chunk lengths from a skewed W x W matrix
(odd values round up), the chunk layout (16-byte aligned regions that do not
overlap), the owner's slot capacity (a power of two >= 2 W max_t), the size
arithmetic at the global caps, and the mode and env parsers.
tests/cpp/lookup_plan_check.cpp holds the checks."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lookup_plan():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    d = tempfile.mkdtemp()
    try:
        exe = os.path.join(d, "lookup_plan")
        subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "lookup_plan_check.cpp")], check=True)
        r = subprocess.run([exe], stdout=subprocess.PIPE)
        out = r.stdout.decode()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    lines = out.strip().splitlines()
    assert lines and all(ln.startswith("ok ") for ln in lines), out
    assert r.returncode == 0
    for name in ("owner_in_range", "owner_uniform", "owner_bits", "pair_max", "chunk_layout",
                 "slot_capacity", "caps_and_overflow", "parsers"):
        assert f"ok {name}" in lines
