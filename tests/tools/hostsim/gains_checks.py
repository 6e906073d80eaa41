"""Gains about a held plan (ilqr_problem_gains) through the C ABI on the host build of the generic kernels (tests/test_gains_cpu.py builds the
library and runs this script in a child process of its own).  Every system shape of tests/gains.py at T = 2, 3, 9, 25 on a ragged batch of 13, a
3-joint chain, a shared keypoint step and a second limit set, for the plans a 0-iteration solve, solve_recursive, solve_al and an early-stopped
solve leave: the oracle's sweep, the bit property, what must not move, the execution tools and the state machine.  The batch solvers and the
cooperative sweeps exist on the device only: tests/test_gpu_gains.py.

    python tests/tools/hostsim/gains_checks.py <libilqr_hostsim.so>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from ilqr_planner_amd import capi  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every call of capi.BatchProblem re-applies the cross-check switches of the environment

from ilqr_planner_amd import workloads  # noqa: E402
from tests import closed_loop as cl  # noqa: E402
from tests import closed_loop_cov as cc  # noqa: E402
from tests import gains as gn  # noqa: E402


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    stats, rep, cov = gn.new_stats(), cl.new_stats(), cc.new_stats()
    for name in gn.SHAPES + gn.EXTRA:
        for T in gn.HORIZONS:
            cfg, desc, inp, systems = gn.make_case(ctx, name, T)
            p = workloads.load_batch(ctx, desc, inp, gn.B)
            try:
                sources = ("zero", "rec") + (("al",) if name in gn.SHAPES else ())
                for source in sources:
                    tag = f"{name} T={T} {source}"
                    plan = gn.check_plan_gains(p, cfg, systems, source, tag, stats)
                    if source == "rec":   # the plans of tests/closed_loop.py: the closed loop about them stays where the replay can follow
                        st = gn.check_execution(ctx, p, cfg, desc, systems, plan, tag, cov)
                        for k in rep:
                            rep[k] = max(rep[k], st[k]) if k.startswith("worst") else rep[k] + st[k]
                gn.check_bits(p, inp, gn.bits_controls(inp), f"{name} T={T} bits")
            finally:
                p.close()
            print(f"{name} T={T}: {', '.join(sources)} and the bit property ok", flush=True)
    name, T, n = gn.STOP_CASE
    cfg, desc, inp, systems = gn.make_case(ctx, name, T)
    p = workloads.load_batch(ctx, desc, inp, gn.B)
    try:
        gn.check_plan_gains(p, dict(cfg, nit=n), systems, "stop", f"{name} T={T} stop", stats, want_stopped=True)
        print(f"{name} T={T}: early-stopped instances ok (iters {p.iters().tolist()})", flush=True)
    finally:
        p.close()
    gn.check_reg_case(ctx, stats)
    print(f"{gn.REG_CASE}: oracle with the same reg, unmoved, bits ok", flush=True)
    gn.check_state_machine(ctx, batch_solvers=False)
    print(f"{stats['n']} instances against the oracle's sweep, {stats['ill']} by its sensitivity (worst ratio {stats['worst_ratio']:.2f}); worst share "
          f"of the tolerance: K {stats['worst_K']:.3f}, d {stats['worst_d']:.3f}; replay: {rep['n']} samples, {rep['ill']} by their sensitivity; "
          f"covariance: {cov['n']} outputs, {cov['ill']} by their sensitivity", flush=True)
    ctx.close()
    print("gains: ok")


if __name__ == "__main__":
    main()
