"""Chains of fewer than 7 joints through the C ABI, on the host: the lane-per-instance kernels and the C-ABI orchestration built with g++ (the
sources and include paths of tests/tools/hostsim/build.sh, without sanitizers), driven by tests/tools/hostsim/narrow_chain_checks.py in a child
process of its own.  FK and the Jacobian of 6- and 3-joint cut Panda chains against the oracle; recursive and AL solves of every PosOrn shape
against the oracle at the native dof; the oracle on the native and the hand-padded 7-joint chain; the exact embedding of the native problem in
the hand-padded 7-joint one; the error texts.  The map of ilqr_dofmap.hpp itself: tests/cpp/dofmap_table_main.cpp."""
import os
import subprocess
import sys

from tests.helpers import build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")
SRC = os.path.join(ROOT, "ilqr_planner_amd", "csrc")


def test_dofmap_table(tmp_path):
    exe = str(tmp_path / "dofmap_table")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + SRC, os.path.join(ROOT, "tests", "cpp", "dofmap_table_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"


def test_narrow_chains_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "narrow_chain_checks.py"), lib], capture_output=True, text=True, timeout=900,
                       cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "narrow chains: ok"
