"""Gains with the AL constraint terms about a held plan (ilqr_problem_gains_al) on the host: k_gains_prepare, k_gains_al_weights, k_kp_derivs, the
generic AL sweep and the C-ABI entry point built with g++ (the sources and include paths of tests/tools/hostsim/build.sh, without sanitizers),
driven by tests/tools/hostsim/gains_al_checks.py in a child process of its own.  The cases and checks of tests/gains_al.py; the device kernels and
the Batch-CP plans: tests/test_gpu_gains_al.py."""
import os
import subprocess
import sys

from tests.helpers import build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")


def test_gains_al_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "gains_al_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "gains_al: ok"
