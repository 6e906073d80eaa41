"""The forward-pass pins of plan_riccati (ilqr_planner_amd/csrc/ilqr_plan.hpp) on the single-integrator systems, checked on the host by a C++
program (tests/cpp/fwd_pin_main.cpp): pin 3 (ILQR_XC_FWD_WG_LDS) selects the old k_forward_wg at any batch size, pin 1 and AUTO beyond 3072
instances select Forward::WaveWg with the register rollout, and no pin changes anything but the forward kernel."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forward_pins(tmp_path):
    exe = str(tmp_path / "fwd_pin")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ilqr_planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fwd_pin_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
