"""CPU unit test of the sumcheck prover's host-side decisions
(csrc/sumcheck_plan.h): the kernel and grid of every large round, the round
the tail starts at on one GPU and sharded, the buffer each round reads and
writes, the io region's layout and the QG_SC_* switch parser are pure functions
of the proof's shape, the device's size and the switches.
tests/cpp/sumcheck_plan_check.cpp pins the 2^20 headline plan, a sop and a
staged plan, the sharded gather rounds with their clamp, the buffer rule for
nvars 1..24 from every first tail round, the io offsets and the parser."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sumcheck_plan():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    d = tempfile.mkdtemp()
    try:
        exe = os.path.join(d, "sumcheck_plan")
        subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "sumcheck_plan_check.cpp")], check=True)
        r = subprocess.run([exe], stdout=subprocess.PIPE)
        out = r.stdout.decode()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    lines = out.strip().splitlines()
    assert lines and all(ln.startswith("ok ") for ln in lines), out
    assert r.returncode == 0
    for name in ("headline_2p20", "sop_2p18", "staged_2p16", "tail_geometry",
                 "sharded_gather_round", "sharded_gather_round_clamp", "buffer_rule",
                 "io_layout", "switch_parser"):
        assert f"ok {name}" in lines
