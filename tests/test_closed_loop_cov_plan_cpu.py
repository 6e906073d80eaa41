"""The kernel selection of the closed-loop covariance (plan_closed_loop_cov, ilqr_planner_amd/csrc/ilqr_closed_loop_plan.hpp) is a pure
function: its table for every system, batch sizes from 1 to 2^20 and the generic pin are checked on the host by a C++ program
(tests/cpp/closed_loop_cov_plan_main.cpp) that includes nothing but that header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_closed_loop_cov_plan_table(tmp_path):
    exe = str(tmp_path / "closed_loop_cov_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ilqr_planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "closed_loop_cov_plan_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
