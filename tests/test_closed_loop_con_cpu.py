"""Closed-loop executions and covariance judged against the AL constraint rows on the host: the generic kernels and the C-ABI entry points
built with g++ exactly as tests/test_closed_loop_cpu.py builds them (no sanitizer, nothing preloaded), driven by
tests/tools/hostsim/closed_loop_con_checks.py in a child process of its own.  The device kernels: tests/test_gpu_closed_loop_con.py."""
import os
import subprocess
import sys

from tests.helpers import build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")


def test_closed_loop_con_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "closed_loop_con_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "closed loop con: ok"
    print("\n".join(r.stdout.strip().splitlines()[-5:]))
