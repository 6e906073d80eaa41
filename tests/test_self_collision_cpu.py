"""Self-collision pairs (ilqr_clr_robot::n_self / self_pair) in the clearance calls and the obstacle terms on the host: clr_state and obs_state
with their self-pair blocks, the kernels above them and the C-ABI entry points built with g++ (the sources and include paths of
tests/tools/hostsim/build.sh, without sanitizers), driven by tests/tools/hostsim/self_collision_checks.py in a child process of its own.  The cases
and checks of tests/self_collision.py against the references of tests/self_collision_reference.py; the device kernels and the cooperative path:
tests/test_gpu_self_collision.py."""
import os
import subprocess
import sys

from tests.helpers import build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")


def test_self_collision_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "self_collision_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "self-collision: ok"
