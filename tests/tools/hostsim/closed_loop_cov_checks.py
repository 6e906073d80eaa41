"""Analytic covariance of the closed loop (ilqr_problem_closed_loop_cov) through the C ABI on the host build of the generic kernel k_cl_cov and of
k_cl_cov_kp (tests/test_closed_loop_cov_cpu.py builds the library and runs this script in a child process of its own).  Every system shape of
tests/closed_loop.py at T = 2, 3, 9, 25 on a ragged batch of 13, held to the checks of tests/closed_loop_cov.py; the 32-bit refusals need a
problem that only fits a device.

    python tests/tools/hostsim/closed_loop_cov_checks.py <libilqr_hostsim.so>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from ilqr_planner_amd import capi  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every call of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import closed_loop as cl  # noqa: E402
from tests import closed_loop_cov as cc  # noqa: E402


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    stats, jac = cc.new_stats(), [0.0]
    for name in cl.SHAPES + cl.EXTRA:
        for T in cc.HORIZONS:
            print(cc.check_case(ctx, name, T, stats=stats, jac_worst=jac), flush=True)
    for name in ("C2", "C2nd", "C4", "chain3"):
        cc.check_cut_out(ctx, name)
        print(f"{name}: cut-out ok", flush=True)
    for name in cc.SAMPLED:
        worst, worst_open = cc.check_sampled(ctx, name)
        print(f"{name}: sample covariance within {worst:.2f} standard deviations of Sigma (open loop: {worst_open:.1f})", flush=True)
    cc.check_interfaces(ctx, cc.host_pointer_call)  # on this build a "device" pointer is a host pointer
    print(f"{stats['n']} outputs, {stats['ill']} by their sensitivity (worst ratio {stats['worst_ratio']:.2f}); worst deviations within the bound: "
          + ", ".join(f"{f} {stats[f]:.3e}" for f in cc.FIELDS) + f"; [A B] from the oracle's step by at most {jac[0]:.3e}", flush=True)
    ctx.close()
    print("closed loop cov: ok")


if __name__ == "__main__":
    main()
