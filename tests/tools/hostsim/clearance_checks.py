"""Clearance of plans and trajectories (ilqr_problem_clearance, ilqr_clearance_trajectories) through the C ABI on the host build
(tests/test_clearance_cpu.py builds the library and runs this script in a child process of its own): clr_state, k_clr_plan, k_clr_traj, k_clr_fold
and k_clr_stats as plain C++, with the _dev forms on host pointers.  Every case and check of tests/clearance.py but the plan left by two halves on
two streams and the class level, which exist on the device only: tests/test_gpu_clearance.py.

    python tests/tools/hostsim/clearance_checks.py <libilqr_hostsim.so>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from ilqr_planner_amd import capi  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every call of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import clearance as clr  # noqa: E402
from tests import multistart as ms  # noqa: E402


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    arrays = ms.HostArrays()
    for name in clr.CASES:
        clr.check_reference(ctx, arrays, name)
    print("reference ok", flush=True)
    clr.check_ties(ctx, arrays)
    clr.check_boundary(ctx, arrays)
    clr.check_bad_steps(ctx, arrays)
    print("ties, boundary, bad steps ok", flush=True)
    for cname, system, T, B, tps in clr.FORMS:
        clr.check_forms(ctx, arrays, cname, system, T, B, tps, f"{cname} {system} T={T} B={B}")
    clr.check_executions(ctx, arrays)
    print("forms, executions ok", flush=True)
    clr.check_selection(ctx, arrays)
    clr.check_untouched(ctx, arrays)
    clr.check_refusals(ctx, arrays)
    ctx.close()
    print("clearance: ok")


if __name__ == "__main__":
    main()
