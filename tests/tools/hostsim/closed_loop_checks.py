"""Batched closed-loop rollouts (ilqr_problem_closed_loop) through the C ABI on the host build of the generic kernel k_closed_loop
(tests/test_closed_loop_cpu.py builds the library and runs this script in a child process of its own).  Every system shape of tests/horizons.py
plus a 3-joint chain, a shared-step case and binding joint limits, at T = 2, 3, 9, 25 on a ragged batch of 13 with S = 1, 3 and 5, held to the
checks (a) to (d) of tests/closed_loop.py; then the error texts and the device-pointer entry point.

    python tests/tools/hostsim/closed_loop_checks.py <libilqr_hostsim.so>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ilqr_planner_amd import capi  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every call of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import closed_loop as cl  # noqa: E402

HORIZONS = (2, 3, 9, 25)
SAMPLES = (1, 3, 5)


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    stats = cl.new_stats()
    for name in cl.SHAPES + cl.EXTRA:
        for T in HORIZONS:
            print(cl.check_case(ctx, name, T, SAMPLES, stats=stats), flush=True)
    cl.check_interfaces(ctx, cl.host_pointer_call)  # on this build a "device" pointer is a host pointer
    print(f"{stats['n']} samples, {stats['ill']} ill-conditioned (worst ratio {stats['worst_ratio']:.2f} of {cl.ILL_FACTOR:g}); worst deviation of "
          f"the others: X {stats['worst_X']:.3e}, U {stats['worst_U']:.3e}, J {stats['worst_J']:.3e} relative", flush=True)
    ctx.close()
    print("closed loop: ok")


if __name__ == "__main__":
    main()
