"""CPU unit test of the MSM launch plan (csrc/msm_plan.h): the sort geometry,
chunk length, tree width, accumulate form, LDS sizes and scatter grids that
msm_accumulate_phase launches with are a pure function of the MSM's shape and
the tuning overrides.  tests/cpp/msm_plan_check.cpp pins whole plans of the
shapes the product runs (the 2^24 headline, a HyperPlonk opening on a side
stream, many-window SRS, a one-shot window), the overrides that name no kernel
instantiation, and the override parser."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_msm_plan():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    d = tempfile.mkdtemp()
    try:
        exe = os.path.join(d, "msm_plan")
        subprocess.run([gxx, "-O1", "-std=c++17", "-Wall", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "msm_plan_check.cpp")], check=True)
        r = subprocess.run([exe], stdout=subprocess.PIPE)
        out = r.stdout.decode()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    lines = out.strip().splitlines()
    assert lines and all(ln.startswith("ok ") for ln in lines), out
    assert r.returncode == 0
    for name in ("headline_2p24_c20", "headline_grid_a_0", "side_2p20_c20", "lone_2p20_c20",
                 "lone_2p15_c13", "lone_2p15_c13_tile_1024_unsupported", "lone_2p22_c13",
                 "oneshot_window_2p20_c20", "geometry_without_instantiation_invalid",
                 "instantiated_geometries_accepted", "forced_scatter_grids",
                 "accumulate_overrides", "override_parser"):
        assert f"ok {name}" in lines
