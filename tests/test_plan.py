"""CPU test of the path decisions in csrc/mvc_plan.h (which kernel instance
runs for a state shape): a stand-alone host program
(tests/plan_driver.cpp, no HIP) prints the phase-A plan, the repair's run-kernel
layouts and the run-kernel instances over boundary shapes and every MVC_PATH
key, and the output must equal the fixture recorded from the decisions as the
samplers made them before they moved into the header.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_golden.txt")


@pytest.fixture(scope="module")
def plan_lines(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("plan") / "plan_driver"
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "multiview-clustering_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", str(exe), os.path.join(ROOT, "tests", "plan_driver.cpp")], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()


def test_plan_matches_golden(plan_lines):
    want = open(GOLDEN).read().splitlines()
    assert len(plan_lines) == len(want)
    for k, (a, b) in enumerate(zip(plan_lines, want)):
        assert a == b, f"line {k + 1}"


def _zpath(line):
    return int(line.split(" | ")[1].split()[2])


def _case(lines, head):
    hits = [ln for ln in lines if ln.startswith(head + " |")]
    assert hits, head
    return hits[0]


def test_plan_agrees_with_recorded_paths(plan_lines):
    """Facts the project records elsewhere: the bench's configs[3] shape runs
    the all-views MFMA producer and the register draw (profiles/r6an_bench.json),
    New_Simulation the lane loop (zpath & 256), and the zpath bits the GPU
    tests assert at their shapes (test_gpu_parity.py)."""
    z = _zpath(_case(plan_lines, "n=1000000 V=4 D=128 T=64 K=64h SP=32 s1t=1 cu=256"))
    assert z & 2 and z & 4 and z & 16 and not z & (32 | 64 | 128)
    assert _zpath(_case(plan_lines, "n=200 V=5 D=1 T=4 K=2u SP=0 s1t=0 cu=256")) == 32 | 256
    # test_zpath2_vs_oracle: MFMA producer; the register draw iff T <= 64; zdraw=row -> 128, zdraw=lds -> neither
    for head, reg in (("n=3001 V=4 D=64 T=16 K=16h SP=16 s1t=1 cu=256", True),
                      ("n=5000 V=3 D=32 T=200 K=32h SP=8 s1t=1 cu=256", False)):
        z = _zpath(_case(plan_lines, head + " [generic=0,zdraw=reg,lpall=1]"))
        assert z & 3 == 2 and bool(z & 4) == reg
        z = _zpath(_case(plan_lines, head + " [generic=0,zdraw=row,lpall=1]"))
        assert z & 3 == 2 and z & 128 and not z & 4
        z = _zpath(_case(plan_lines, head + " [generic=0,zdraw=lds,lpall=1]"))
        assert z & 3 == 2 and not z & (4 | 128)
        assert _zpath(_case(plan_lines, head + " [generic=1]")) & 3 == 0
    # test_many_views_row_draw_gate: more than 16 views never take the row draw
    assert not _zpath(_case(plan_lines, "n=1200 V=18 D=16 T=96 K=8h SP=0 s1t=0 cu=256 [zdraw=row]")) & 128
    # test_dish_block_producer: K_v > 64, and big=1 on a tiled shape
    assert _zpath(_case(plan_lines, "n=6000 V=3 D=32 T=128 K=128h SP=8 s1t=0 cu=256")) & 64
    assert _zpath(_case(plan_lines, "n=4100 V=4 D=64 T=64 K=64h SP=16 s1t=1 cu=256 [big=1]")) & 64
    assert _zpath(_case(plan_lines, "n=3000 V=2 D=256 T=80 K=80h SP=64 s1t=0 cu=256 [big=1,big_sp=runtime]")) & 64
