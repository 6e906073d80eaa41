"""plan_riccati with obstacle terms (PlanIn::obstacles, ilqr_planner_amd/csrc/ilqr_plan.hpp): the generic kernels for init, sweep and forward under
every pin (tests/cpp/obstacle_plan_main.cpp), and the existing decision table unchanged with the flag off (tests/cpp/plan_table_main.cpp as it
is, built against the same header)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("main", ["obstacle_plan_main", "plan_table_main"])
def test_plan_with_and_without_obstacles(tmp_path, main):
    exe = str(tmp_path / main)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ilqr_planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", main + ".cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
