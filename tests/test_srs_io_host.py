"""CPU unit test of the SRS import's host-only helpers (csrc/srs_io.h): the
byte-size and range bounds (overflow at SIZE_MAX), the packed "lowest bad
point" word the decode kernel's atomicMin folds into, and the message of
qg_last_error.  tests/cpp/srs_io_check.cpp holds the checks; it is a
stand-alone program built with AddressSanitizer and UBSan."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_srs_io_host():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    d = tempfile.mkdtemp()
    try:
        exe = os.path.join(d, "srs_io_check")
        subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "srs_io_check.cpp")], check=True)
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        out = r.stdout.decode()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    lines = out.strip().splitlines()
    assert lines and all(ln.startswith("ok ") for ln in lines), out + r.stderr.decode()
    assert r.returncode == 0, r.stderr.decode()
    for name in ("point_bytes", "bytes_checked", "range", "bad_word", "messages"):
        assert f"ok {name}" in lines
