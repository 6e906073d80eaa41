"""The sweep pin 7 (ILQR_XC_SWEEP_SI_WG_PREP) and the field RiccatiPlan::si_prep of plan_riccati (ilqr_planner_amd/csrc/ilqr_plan.hpp), checked on
the host by a C++ program (tests/cpp/sweep_prep_pin_main.cpp): the preparing-wave form of k_backward_si_dpp is chosen only where the I/O-wave form
is (si_prep => si_io => si_wg), pin 7 acts as pin 6 elsewhere, pins 4, 5 and 6 turn it off, AUTO adds it from SI_PREP_MIN_BATCH launched instances
where it takes the I/O wave, split halves and the 8-lane grouping never get it under AUTO, and every other field of the plan stays as it was."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_prep_pins(tmp_path):
    exe = str(tmp_path / "sweep_prep_pin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ilqr_planner_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sweep_prep_pin_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
