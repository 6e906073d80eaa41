"""Obstacle terms of the stage cost (ilqr_problem_set_obstacles, ilqr_problem_obstacle_terms) through the C ABI on the host build
(tests/test_obstacles_cpu.py builds the library and runs this script in a child process of its own): obs_state, k_obs_derivs, k_obs_query and the
OBS forms of k_init_rollout / k_backward / k_forward as plain C++, with the _dev forms on host pointers.  Every case and check of
tests/obstacles.py; the device kernels: tests/test_gpu_obstacles.py.

    python tests/tools/hostsim/obstacle_checks.py <libilqr_hostsim.so> [file that receives the worst ratio of check (a)]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from ilqr_planner_amd import capi  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every call of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import multistart as ms  # noqa: E402
from tests import obstacles as ob  # noqa: E402


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    arrays = ms.HostArrays()
    ob.check_reference_gradient(ctx)
    worst = max(ob.check_terms(ctx, arrays, name) for name in ob.CASES)
    print(f"terms ok: worst ratio to the tolerance {worst:.3e}", flush=True)
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write(f"{worst:.3e}\n")
    for cname, system, T, B in (("panda", "po1", 9, 13), ("gen4", "pot2", 3, 5)):
        ob.check_inert(ctx, cname, system, T, B, f"inert {cname} {system}", unpinned=False)
    print("inert ok", flush=True)
    for cname, system, T, B, al, nit in ob.ITER_CASES:
        ob.check_iterations(ctx, cname, system, T, B, al, nit, f"iterations {cname} {system} T={T} al={al} nit={nit}")
    print("iterations ok", flush=True)
    ob.check_bites(ctx)
    print("bites ok", flush=True)
    for cname, system, T, B, al in (("panda", "po1", 9, 13, False), ("gen4", "pot2", 3, 5, False), ("panda", "po1", 9, 13, True), ("gen7", "po2", 3, 5, True)):
        ob.check_gains(ctx, cname, system, T, B, al, f"gains {cname} {system} al={al}")
    ob.check_untouched(ctx, arrays)
    ob.check_refusals(ctx, arrays, batch_solvers=False)
    ctx.close()
    print("obstacles: ok")


if __name__ == "__main__":
    main()
