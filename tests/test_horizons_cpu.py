"""Short and odd horizons on the host: the lane-per-instance kernels and the C-ABI orchestration built with g++ (the sources and include paths
of tests/tools/hostsim/build.sh, without sanitizers), driven by tests/tools/hostsim/horizon_checks.py in a child process of its own.  Every
system shape (C2, C2r, C3, C2nd, C2ndal, C4t1, C4, C4al, C1j, C1t, C2h, C2hl) at T = 2 .. 25 and the keypoint placements of tests/horizons.py, gated by its
check_case (gains at every step, the parity proof, trajectories); the multipliers, the tracking law at t = T - 2 and the warm start by
T - 1 steps at T = 2, 3 and 9.  The device kernels at the same horizons: tests/test_gpu_horizons.py."""
import os
import subprocess
import sys

from tests.helpers import build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")


def test_horizons_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "horizon_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "horizons: ok"
