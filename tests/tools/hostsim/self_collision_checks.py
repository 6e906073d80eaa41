"""Self-collision pairs (ilqr_clr_robot::n_self / self_pair) through the C ABI on the host build (tests/test_self_collision_cpu.py builds the
library and runs this script in a child process of its own): clr_state and obs_state with their self-pair blocks as plain C++, under the clearance
calls, k_obs_derivs, k_obs_query and the OBS forms of the generic kernels, with the _dev forms on host pointers.  Every check of
tests/self_collision.py but those of the cooperative path, which the host build does not have; the device kernels: tests/test_gpu_self_collision.py.

    python tests/tools/hostsim/self_collision_checks.py <libilqr_hostsim.so> [file that receives the worst ratios of checks (a), (b), (d)]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from ilqr_planner_amd import capi  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every call of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import multistart as ms  # noqa: E402
from tests import self_collision as sc  # noqa: E402


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    arrays = ms.HostArrays()
    sc.check_reference_gradient(ctx)
    worst_a = max(sc.check_clearance(ctx, arrays, name) for name in sc.CLR_CASES)
    sc.check_duplicate_anchor(ctx, arrays)
    sc.check_forms(ctx, arrays, "panda", "po1", 9, 13, 1, 5, 7, 3, True, "forms panda po1")
    sc.check_forms(ctx, arrays, "gen4", "pot2", 3, 70, 70, 5, 7, 3, False, "forms gen4 pot2")
    sc.check_forms(ctx, arrays, "gen7", "pot2", 2, 70, 5, 32, 64, 8, True, "forms gen7 pot2, 32 spheres")
    print(f"clearance ok: worst ratio to the tolerance {worst_a:.3e}", flush=True)
    worst_b = max(sc.check_terms(ctx, arrays, name) for name in sc.CASES)
    print(f"terms ok: worst ratio to the tolerance {worst_b:.3e}", flush=True)
    for cname, system, T, B in (("panda", "po1", 9, 13), ("gen4", "pot2", 3, 5)):
        sc.check_inert(ctx, cname, system, T, B, f"inert {cname} {system}")
    print("inert ok", flush=True)
    worst_d = dict(K=0.0, d=0.0, cost=0.0)
    for cname, system, T, B, al, nit, world in sc.ITER_CASES:
        w = sc.check_iterations(ctx, cname, system, T, B, al, nit, world, f"iterations {cname} {system} T={T} al={al} nit={nit} world={world}")
        worst_d = {k: max(v, w[k]) for k, v in worst_d.items()}
    print("iterations ok", flush=True)
    sc.check_bites(ctx)
    print("bites ok", flush=True)
    sc.check_selection(ctx, arrays)
    print("selection ok", flush=True)
    for cname, system, T, B, al in (("panda", "po1", 9, 13, False), ("gen4", "pot2", 3, 5, False), ("panda", "po1", 9, 13, True), ("gen7", "po2", 3, 5, True)):
        sc.check_gains(ctx, cname, system, T, B, al, f"gains {cname} {system} al={al}")
    sc.check_refusals(ctx, arrays)
    ctx.close()
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(f"host build: (a) clr, clr_min {worst_a:.3e}; (b) terms {worst_b:.3e}; (d) K {worst_d['K']:.3e}, d {worst_d['d']:.3e}, cost {worst_d['cost']:.3e}\n")
    print("self-collision: ok")


if __name__ == "__main__":
    main()
