"""CPU unit test of the sharded openings' slice geometry (csrc/open_plan.h),
the integers mle_open_batch_sharded and ipa_prove_sharded decide on: for
W in {1, 2, 4, 8}, L in {1, 2, 16} and every global trimmed length n in
[0, W L], a rank's live part of a polynomial and of its quotient against a
brute-force count of the indices in the slice; the global length rebuilt from
brute-force-trimmed slices of 0/1 patterns (top slices all zero included);
and the group-wide "fits" decision against the conjunction over ranks for
every assignment of shard sizes from {0, L - 1, L}.
tests/cpp/open_plan_check.cpp holds the checks; it is a stand-alone program
built with AddressSanitizer and UBSan."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_open_plan():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    d = tempfile.mkdtemp()
    try:
        exe = os.path.join(d, "open_plan")
        subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "open_plan_check.cpp")], check=True)
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        out = r.stdout.decode()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    lines = out.strip().splitlines()
    assert lines and all(ln.startswith("ok ") for ln in lines), out + r.stderr.decode()
    assert r.returncode == 0, r.stderr.decode()
    for name in ("live_qlive", "global_len", "fits"):
        assert f"ok {name}" in lines
