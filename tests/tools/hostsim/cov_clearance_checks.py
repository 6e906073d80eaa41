"""Clearance under the closed-loop covariance (ilqr_problem_closed_loop_cov_clr) through the C ABI on the host build
(tests/test_cov_clearance_cpu.py builds the library and runs this script in a child process of its own): cov_clr_state, k_cov_clr and
k_cov_clr_fold as plain C++ behind the generic covariance kernel, with the _dev forms on host pointers.  Every check of tests/cov_clearance.py
under the generic pin; k_cl_cov_rows and the device kernels: tests/test_gpu_cov_clearance.py.

    python tests/tools/hostsim/cov_clearance_checks.py <libilqr_hostsim.so> [file that receives the worst ratios of check (a)]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from ilqr_planner_amd import capi  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every call of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import cov_clearance as cc  # noqa: E402
from tests import multistart as ms  # noqa: E402


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    arrays = ms.HostArrays()
    worst = dict(var=0.0, z=0.0)
    for name in cc.CASES:
        w = cc.check_values(ctx, arrays, name)
        worst = {k: max(v, w[k]) for k, v in worst.items()}
    print(f"values ok: worst ratio to the bound: clr_var {worst['var']:.3e}, clr_z {worst['z']:.3e}", flush=True)
    cc.check_cov_con_unchanged(ctx)
    cc.check_exact(ctx, arrays)
    print("exact ok", flush=True)
    cc.check_bad(ctx, arrays)
    cc.check_selection(ctx, arrays)
    print("selection ok", flush=True)
    cc.check_untouched(ctx, arrays)
    cc.check_refusals(ctx, arrays)
    print("refusals ok", flush=True)
    cc.check_meaning(ctx, arrays)
    ctx.close()
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(f"host build: (a) clr_var {worst['var']:.3e}, clr_z {worst['z']:.3e} of their bounds\n")
    print("cov clearance: ok")


if __name__ == "__main__":
    main()
