"""Analytic covariance of the closed loop on the host: the generic kernel k_cl_cov, k_cl_cov_kp and the C-ABI entry points built with g++ (the
sources and include paths of tests/tools/hostsim/build.sh, without sanitizers), driven by tests/tools/hostsim/closed_loop_cov_checks.py in a
child process of its own.  Every system shape of tests/closed_loop.py at T = 2, 3, 9, 25, B = 13 against the NumPy recursion, the Jacobian
against the oracle's step, the exact properties, the sampled path and the refusals (tests/closed_loop_cov.py).  The device kernels:
tests/test_gpu_closed_loop_cov.py."""
import os
import subprocess
import sys

from tests.helpers import build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")


def test_closed_loop_cov_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "closed_loop_cov_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "closed loop cov: ok"
