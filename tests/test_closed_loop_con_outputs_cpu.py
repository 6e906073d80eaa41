"""Every subset of the outputs that ilqr_problem_closed_loop_report_con and ilqr_problem_closed_loop_cov_con add gives the same bytes, through
host and through device pointers (tests/cpp/closed_loop_con_outputs_main.cpp): the staging layout and the workspaces of closed_loop and
closed_loop_cov (ilqr_planner_amd/csrc/ilqr_capi_closed_loop.cpp) for every combination of the new outputs.  The program is built from the host sources of
tests/helpers.hostsim_sources with the address and undefined-behaviour sanitizers into an executable of its own and run as a child process.

Calls made, S = 2: _report_con (2 x 2^4 - 1 (nothing asked for)) subsets x 2 (noise, w) = 62; _cov_con 2 x 2^2 - 1 = 7; each through host and
through device pointers: 2 x 69 = 138."""
import os
import subprocess

from tests.helpers import ROOT, hostsim_sources

CASES = 2 * (2 * (2 * 2 ** 4 - 1) + (2 * 2 ** 2 - 1))


def test_every_subset_of_the_constraint_outputs_gives_the_same_bytes(tmp_path):
    hostsim = os.path.join(ROOT, "tests", "tools", "hostsim")
    src = os.path.join(ROOT, "ilqr_planner_amd", "csrc")
    exe = str(tmp_path / "closed_loop_con_outputs")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + hostsim,
                           "-I" + src, "-I" + os.path.join(ROOT, "include"), "-Wno-unused-result", "-x", "c++",
                           *hostsim_sources(), os.path.join(ROOT, "tests", "cpp", "closed_loop_con_outputs_main.cpp"), "-o", exe])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "panda_chain.urdf")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok", r.stdout + r.stderr
    assert lines[-2] == f"cases: {CASES}", r.stdout
