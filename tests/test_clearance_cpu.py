"""Clearance of plans and trajectories (ilqr_problem_clearance, ilqr_clearance_trajectories) on the host: clr_state, k_clr_plan, k_clr_traj,
k_clr_fold, k_clr_stats and the C-ABI entry points built with g++ (the sources and include paths of tests/tools/hostsim/build.sh, without
sanitizers), driven by tests/tools/hostsim/clearance_checks.py in a child process of its own.  The cases and checks of tests/clearance.py against
the 50-digit reference of tests/clearance_reference.py; the device kernels: tests/test_gpu_clearance.py."""
import os
import subprocess
import sys

from tests.helpers import build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")


def test_clearance_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "clearance_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "clearance: ok"
