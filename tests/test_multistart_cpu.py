"""Multi-start solves (ilqr_problem_adopt, ilqr_problem_spread_controls, ilqr_problem_select, ilqr_problem_get_at) on the host: k_adopt_rows,
k_spread_controls, k_select_group, k_get_at and the C-ABI entry points built with g++ (the sources and include paths of
tests/tools/hostsim/build.sh, without sanitizers), driven by tests/tools/hostsim/multistart_checks.py in a child process of its own.  The cases and
checks of tests/multistart.py; the device kernels: tests/test_gpu_multistart.py."""
import os
import subprocess
import sys

from tests.helpers import build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")


def test_multistart_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "multistart_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "multistart: ok"
