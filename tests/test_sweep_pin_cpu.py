"""The sweep pins 4 (ILQR_XC_SWEEP_SI_WAVE) and 5 (ILQR_XC_SWEEP_SI_WG) of plan_riccati (ilqr_planner_amd/csrc/ilqr_plan.hpp), checked on the host by
a C++ program (tests/cpp/sweep_pin_main.cpp): they choose the form of k_backward_si_dpp only where the sweep is Sweep::SiDpp with 16 lanes per
instance, AUTO switches at SI_WG_MIN_BATCH launched instances, the pins mfma / rows and every other field of the plan stay as they were."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_pins(tmp_path):
    exe = str(tmp_path / "sweep_pin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ilqr_planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "sweep_pin_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
