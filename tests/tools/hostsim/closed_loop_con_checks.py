"""Closed-loop executions and covariance judged against the AL constraint rows (ilqr_problem_closed_loop_report_con,
ilqr_problem_closed_loop_cov_con) through the C ABI on the host build of the generic kernels k_closed_loop (CON), k_closed_loop_con_stats,
k_closed_loop_outcome_con and k_cl_cov (tests/test_closed_loop_con_cpu.py builds the library and runs this script in a child process of its
own).  Every case of tests/closed_loop_con.py at T = 2, 3, 9, 10 on a ragged batch of 13 with S = 1, 4, 5, 17, held to its checks (1)-(7); the
comparisons of two device kernels need the device.

    python tests/tools/hostsim/closed_loop_con_checks.py <libilqr_hostsim.so>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from ilqr_planner_amd import capi  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every call of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import closed_loop_con as cc  # noqa: E402

COMBOS = ((2, (1, 4)), (3, (5,)), (9, (4, 17)), (10, (5,)))


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    worst = dict(con_max=0.0, con_var=0.0)
    only = sys.argv[2:]
    for case in cc.CASES:
        if only and case not in only:
            continue
        for T, samples in COMBOS:
            print(cc.check_case(ctx, case, T, samples, worst=worst), flush=True)
    for case in ("C3-m4", "C4t1al-m2-control-per_step"):
        cc.check_cut_out(ctx, case)
        print(f"{case}: cut-out ok", flush=True)
    cc.check_violated_plan(ctx)
    print(f"sampled against analytic: {cc.check_sampled_against_analytic(ctx):.3f} of the allowed deviation", flush=True)
    cc.check_interfaces(ctx, cc.host_pointer_call, cc.host_pointer_cov_call)  # on this build a "device" pointer is a host pointer
    ctx.close()
    print("closed loop con: ok")


if __name__ == "__main__":
    main()
