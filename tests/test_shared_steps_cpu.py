"""Keypoints that share a timestep, on the host.  The step table of ilqr_steps.hpp and the plan rows that send shared steps to the generic
kernels (tests/cpp/step_table_main.cpp, g++); the lane-per-instance kernels and the C-ABI orchestration built with g++ (the sources and include
paths of tests/tools/hostsim/build.sh, without sanitizers), driven by tests/tools/hostsim/shared_step_checks.py in a child process of its own:
the exact reductions of tests/shared_steps.py and the last-wins rule of a plain System against the oracle, the batch solvers' error text;
tests/cpp/shared_steps_main.cpp (general mixtures: the lowering against the host loop over the virtuals) linked against the same build.  On the device:
tests/test_gpu_shared_steps.py."""
import os
import subprocess
import sys

from tests.helpers import build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")
SRC = os.path.join(ROOT, "ilqr_planner_amd", "csrc")


def test_step_table(tmp_path):
    exe = str(tmp_path / "step_table")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + SRC, os.path.join(ROOT, "tests", "cpp", "step_table_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"


def test_shared_steps_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "shared_step_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "shared steps: ok"


def test_mixtures_device_against_host_loop_on_host_build(tmp_path):
    """tests/cpp/shared_steps_main.cpp linked against the host build (its generic kernels; the LQT entry points refused): an object frame, a
    dead zone, a joint and two PosOrn keypoints with different targets on one step, solved through the lowering and over the virtuals."""
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    host = os.path.join(SRC, "host")
    exe = str(tmp_path / "shared_steps")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "shared_steps_main.cpp"), os.path.join(host, "ilqr_host.cpp"),
                           os.path.join(host, "ilqr_host_loop.cpp"), os.path.join(HOSTSIM, "lqt_stubs.cpp"), "-o", exe, lib,
                           "-Wl,-rpath," + str(tmp_path)])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "panda_chain.urdf"), "generic"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
