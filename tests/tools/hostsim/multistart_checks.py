"""Multi-start solves (ilqr_problem_adopt, ilqr_problem_spread_controls, ilqr_problem_select, ilqr_problem_get_at) through the C ABI on the host
build of the generic kernels (tests/test_multistart_cpu.py builds the library and runs this script in a child process of its own): k_adopt_rows,
k_spread_controls, k_select_group in its one-lane form and k_get_at, with the _dev forms on host pointers.  Every system of tests/multistart.py at
T = 2, 3, 9 and the group shapes (13, 1), (5, 3), (1, 70); the planted-winner condition is judged by the oracle here.  The lane-group forms of
k_select_group and the split plans exist on the device only: tests/test_gpu_multistart.py.

    python tests/tools/hostsim/multistart_checks.py <libilqr_hostsim.so>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from ilqr_planner_amd import capi  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every call of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import multistart as ms  # noqa: E402


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    arrays = ms.HostArrays()
    for name in ms.SYSTEMS:
        for T in ms.HORIZONS:
            for G, S in ms.GROUPS:
                tag = f"{name} T={T} G={G} S={S}"
                ms.check_select(ctx, arrays, name, T, G, S, tag)
                ms.check_spread(ctx, name, T, G, S, tag)
            ms.check_get_at(ctx, arrays, name, T, 13, f"{name} T={T}")
            ms.check_adopt(ctx, arrays, name, T, 13, 15, f"{name} T={T} adopt 13 <- 15")
            ms.check_adopt(ctx, arrays, name, T, 70, 5, f"{name} T={T} adopt_dev 70 <- 5", dev_form=True)
            print(f"{name} T={T}: select, spread, get_at, adopt ok", flush=True)
    ms.check_adopt_refusals(ctx, "refusals")
    ms.check_adopt_dev_clamps(ctx, arrays, "clamp")
    for name in ms.PIPELINE:
        cfg, desc, inp, Uconv = ms.planted(ctx, name, 9, 5)
        ms.check_planted_condition(name, cfg, inp, Uconv, f"{name} planted")
        ms.check_pipeline(ctx, arrays, cfg, desc, inp, Uconv, 3, f"{name} pipeline G=5 S=3")
        print(f"{name}: planted winner ok", flush=True)
    ctx.close()
    print("multistart: ok")


if __name__ == "__main__":
    main()
