"""Closed-loop rollouts with a report on the host: the generic kernel k_closed_loop with its report stores, k_closed_loop_kp_err,
k_closed_loop_kp_stats, k_closed_loop_outcome and the C-ABI entry points built with g++ exactly as tests/test_closed_loop_cpu.py builds them,
driven by tests/tools/hostsim/closed_loop_report_checks.py in a child process of its own.  The device kernels:
tests/test_gpu_closed_loop_report.py."""
import os
import subprocess
import sys

from tests.helpers import build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")


def test_closed_loop_report_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "closed_loop_report_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "closed loop report: ok"
    print("\n".join(r.stdout.strip().splitlines()[-5:]))
