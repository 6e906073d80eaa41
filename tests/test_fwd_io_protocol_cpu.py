"""The hand-off protocol of k_forward_reg's helper-wave form, run as a host model (tests/cpp/fwd_io_protocol_main.cpp) on the formulas of
ilqr_planner_amd/csrc/ilqr_fwd_io_plan.hpp, the header the kernel includes: under random and adversarial interleavings of the seven waves, for
every subset of dead chain waves and every horizon up to three ring lengths, every step is stored, no slot is overwritten before its last reader
has read it and no wave is blocked forever."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forward_io_protocol(tmp_path):
    exe = str(tmp_path / "fwd_io_protocol")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ilqr_planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fwd_io_protocol_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
