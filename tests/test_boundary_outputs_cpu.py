"""The host / _dev pairs of the C ABI outside the closed loop give the same bytes whichever outputs are asked for, through host and through device
pointers (tests/cpp/boundary_outputs_main.cpp): the staging layouts of get_X / get_U / get_cost, track, get_at, select, adopt, the clearance calls
and obstacle_terms (ilqr_planner_amd/csrc/ilqr_capi_*.cpp), each array against the all-outputs host call.  The program is built from the host
sources of tests/helpers.hostsim_sources with the address and undefined-behaviour sanitizers into an executable of its own and run as a child
process.

Calls per problem (B = 4, T = 6): the 3 getters; track 2 steps x 2 feed-forward flags = 4; get_at 2^5 - 1 = 31; select 2 group sizes x 2 (score)
x 2 (eligible) x (2^3 - 1) = 56; adopt 4 single bits + 1 combination = 5; clearance 2 forms x 2 (self pairs) x (2^6 - 1) = 252; obstacle_terms
2 (self pairs) x (2^3 - 1) = 14: 365, each through host and through device pointers, the list run forward and backward, on two problems (the
Panda and a four-joint chain): 2 x 2 x 2 x 365 = 2920."""
import os
import subprocess

from tests.helpers import GOLDEN, ROOT, hostsim_sources

CASES = 2 * 2 * 2 * (3 + 2 * 2 + (2 ** 5 - 1) + 2 * 2 * 2 * (2 ** 3 - 1) + 5 + 2 * 2 * (2 ** 6 - 1) + 2 * (2 ** 3 - 1))


def test_every_output_subset_of_the_host_dev_pairs_gives_the_same_bytes(tmp_path):
    hostsim = os.path.join(ROOT, "tests", "tools", "hostsim")
    src = os.path.join(ROOT, "ilqr_planner_amd", "csrc")
    exe = str(tmp_path / "boundary_outputs")
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + hostsim,
                           "-I" + src, "-I" + os.path.join(ROOT, "include"), "-Wno-unused-result", "-x", "c++",
                           *hostsim_sources(), os.path.join(ROOT, "tests", "cpp", "boundary_outputs_main.cpp"), "-o", exe])
    r = subprocess.run([exe, os.path.join(GOLDEN, "panda_chain.urdf"), os.path.join(GOLDEN, "chains", "gen4.urdf")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok", r.stdout + r.stderr
    assert lines[-2] == f"cases: {CASES}", r.stdout
