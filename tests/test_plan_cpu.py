"""The kernel selection of the Riccati solvers (plan_riccati, ilqr_planner_amd/csrc/ilqr_plan.hpp) is a pure function: its decision table,
thresholds included, is checked on the host by a C++ program (tests/cpp/plan_table_main.cpp) that includes nothing but that header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_decision_table(tmp_path):
    exe = str(tmp_path / "plan_table")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ilqr_planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "plan_table_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
