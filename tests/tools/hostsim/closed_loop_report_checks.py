"""Closed-loop rollouts with a report (ilqr_problem_closed_loop_report) through the C ABI on the host build of the generic kernel k_closed_loop
with its report stores and of k_closed_loop_kp_err, k_closed_loop_kp_stats and k_closed_loop_outcome (tests/test_closed_loop_report_cpu.py
builds the library and runs this script in a child process of its own).  Every case of tests/closed_loop_report.py at T = 2, 3, 9 on a ragged
batch of 13 with S = 1, 4, 5 (17 at T = 9), held to its checks (1)-(5) and (7)-(9); (6) needs the device.

    python tests/tools/hostsim/closed_loop_report_checks.py <libilqr_hostsim.so>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from ilqr_planner_amd import capi  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every call of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import closed_loop_report as cr  # noqa: E402

COMBOS = ((2, (1, 4)), (3, (5,)), (9, (4, 17)))


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    worst = dict(err=0.0)
    for name in cr.SHAPES:
        for T, samples in COMBOS:
            print(cr.check_case(ctx, name, T, samples, worst=worst), flush=True)
    for name in ("C2", "C4t1"):
        cr.check_cut_out(ctx, name)
        print(f"{name}: cut-out ok", flush=True)
    cr.check_interfaces(ctx, cr.host_pointer_call)  # on this build a "device" pointer is a host pointer
    print(f"worst deviation of a keypoint error from the reference: {worst['err']:.3e} of its bound", flush=True)
    ctx.close()
    print("closed loop report: ok")


if __name__ == "__main__":
    main()
