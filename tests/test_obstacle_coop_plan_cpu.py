"""plan_riccati with PlanIn::obstacles_coop (ilqr_planner_amd/csrc/ilqr_plan.hpp): the dense cooperative plan for the single-integrator shapes with
obstacle terms, today's plan for every other input (tests/cpp/obstacle_coop_plan_main.cpp).  The existing tables stay as they are
(tests/test_obstacle_plan_cpu.py builds them against the same header)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_with_the_cooperative_obstacle_path(tmp_path):
    exe = str(tmp_path / "obstacle_coop_plan_main")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ilqr_planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "obstacle_coop_plan_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
