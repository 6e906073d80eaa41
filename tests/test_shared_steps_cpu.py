"""Keypoints that share a timestep, on the host.  The step table of ilqr_steps.hpp and the plan rows that send shared steps to the generic
kernels (tests/cpp/step_table_main.cpp, g++); the lane-per-instance kernels and the C-ABI orchestration built with g++ (the sources and include
paths of tests/tools/hostsim/build.sh, without sanitizers), driven by tests/tools/hostsim/shared_step_checks.py in a child process of its own:
the exact reductions of tests/shared_steps.py and the last-wins rule of a plain System against the oracle, the batch solvers' error text;
tests/cpp/shared_steps_main.cpp (general mixtures: the lowering against the host loop over the virtuals) linked against the same build.  On the device:
tests/test_gpu_shared_steps.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")
SRC = os.path.join(ROOT, "ilqr_planner_amd", "csrc")


def test_step_table(tmp_path):
    exe = str(tmp_path / "step_table")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + SRC, os.path.join(ROOT, "tests", "cpp", "step_table_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"


def _host_build(tmp_path):
    lib = str(tmp_path / "libilqr_hostsim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + HOSTSIM, "-I" + SRC, "-Wno-unused-result", "-x", "c++",
                           os.path.join(SRC, "ilqr_kernels.hip"), os.path.join(SRC, "ilqr_capi.cpp"), os.path.join(SRC, "urdf_chain.cpp"),
                           os.path.join(HOSTSIM, "stubs.cpp"), "-o", lib])
    return lib


def test_shared_steps_on_host_build(tmp_path):
    lib = _host_build(tmp_path)
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "shared_step_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "shared steps: ok"


def test_mixtures_device_against_host_loop_on_host_build(tmp_path):
    """tests/cpp/shared_steps_main.cpp linked against the host build (its generic kernels; the LQT entry points refused): an object frame, a
    dead zone, a joint and two PosOrn keypoints with different targets on one step, solved through the lowering and over the virtuals."""
    lib = _host_build(tmp_path)
    host = os.path.join(SRC, "host")
    exe = str(tmp_path / "shared_steps")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "shared_steps_main.cpp"), os.path.join(host, "ilqr_host.cpp"),
                           os.path.join(host, "ilqr_host_loop.cpp"), os.path.join(HOSTSIM, "lqt_stubs.cpp"), "-o", exe, lib,
                           "-Wl,-rpath," + str(tmp_path)])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "panda_chain.urdf"), "generic"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
