"""Obstacle terms of the stage cost (ilqr_problem_set_obstacles, ilqr_problem_obstacle_terms) on the host: obs_state, k_obs_derivs, k_obs_query, the
OBS forms of the generic kernels and the C-ABI entry points built with g++ (the sources and include paths of tests/tools/hostsim/build.sh, without
sanitizers), driven by tests/tools/hostsim/obstacle_checks.py in a child process of its own.  The cases and checks of tests/obstacles.py against
the references of tests/obstacle_reference.py; the device kernels: tests/test_gpu_obstacles.py."""
import os
import subprocess
import sys

from tests.helpers import build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")


def test_obstacles_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "obstacle_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "obstacles: ok"
