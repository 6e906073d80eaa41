"""Clearance under the closed-loop covariance (ilqr_problem_closed_loop_cov_clr) on the host: cov_clr_state, k_cov_clr, k_cov_clr_fold and the C-ABI
entry points built with g++ (the sources and include paths of tests/tools/hostsim/build.sh, without sanitizers), driven by
tests/tools/hostsim/cov_clearance_checks.py in a child process of its own.  The cases and checks of tests/cov_clearance.py against the reference of
tests/cov_clearance_reference.py; the device kernels and k_cl_cov_rows: tests/test_gpu_cov_clearance.py."""
import os
import subprocess
import sys

from tests.helpers import build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")


def test_cov_clearance_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "cov_clearance_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "cov clearance: ok"
