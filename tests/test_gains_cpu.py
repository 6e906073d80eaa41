"""Gains about a held plan (ilqr_problem_gains) on the host: k_gains_prepare, k_kp_derivs, the generic sweep and the C-ABI entry point built with
g++ (the sources and include paths of tests/tools/hostsim/build.sh, without sanitizers), driven by tests/tools/hostsim/gains_checks.py in a child
process of its own.  Every system shape of tests/gains.py at T = 2, 3, 9, 25, B = 13, a 3-joint chain, a shared keypoint step and a second limit
set: the oracle's sweep about the held plan, the bit property, what must not move, the execution tools and the state machine (tests/gains.py).
The device kernels and the batch solvers: tests/test_gpu_gains.py."""
import os
import subprocess
import sys

from tests.helpers import build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")


def test_gains_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "gains_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "gains: ok"
