"""The Riccati solvers away from the default reg, alpha_floor and stop_tol through the C ABI on the host build of the lane-per-instance kernels
(tests/test_solver_constants_cpu.py builds the library and runs this script in a child process of its own).  Every [v1] case of
tests/solver_constants.py -- C2 and C4t1 under each cooperative constant set -- and C2, C3 and C4al under the sets past 16 step sizes, gated by
solver_constants.check_case: the parity proof with the case's constants, gains at every step, trajectories, multipliers, status words.

    python tests/tools/hostsim/solver_constants_checks.py <libilqr_hostsim.so>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from ilqr_planner_amd import capi  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every solve of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import solver_constants as sc  # noqa: E402


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    extra = [dict(name=n, pin="v1", set=s, T=sc.HORIZON[n]) for s in sc.PAST16_SETS for n in ("C2", "C3", "C4al")]
    for c in sc.host_cases() + extra:
        cfg, desc, inp = sc.make(ctx, c)
        print(sc.check_case(ctx, cfg, desc, inp, sc.case_id(c)), flush=True)
    ctx.close()
    print("solver constants: ok")


if __name__ == "__main__":
    main()
