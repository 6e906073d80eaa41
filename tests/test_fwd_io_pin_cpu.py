"""The pin 4 (ILQR_XC_FWD_WG_IO) of plan_riccati (ilqr_planner_amd/csrc/ilqr_plan.hpp) and RiccatiPlan::fwd_io, checked on the host by a C++
program (tests/cpp/fwd_io_pin_main.cpp): the pin selects Forward::WaveWg with k_forward_reg's helper waves on the single-integrator systems at
any batch size and nothing else, pins 1 - 3 never set fwd_io, and AUTO sets it exactly in the committed range of launched batch sizes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forward_io_pin(tmp_path):
    exe = str(tmp_path / "fwd_io_pin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ilqr_planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fwd_io_pin_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
