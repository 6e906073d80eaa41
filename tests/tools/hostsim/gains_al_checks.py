"""Gains with the AL constraint terms about a held plan (ilqr_problem_gains_al) through the C ABI on the host build of the generic kernels
(tests/test_gains_al_cpu.py builds the library and runs this script in a child process of its own): k_gains_prepare, k_gains_al_weights,
k_kp_derivs and the generic AL sweep.  Every case of tests/gains_al.py at T = 2, 3, 9, 25 on a ragged batch of 13, for the plans a 0-iteration
solve and an AL solve of six iterations leave, at the workload's initial penalty and at the one the solve ends with: the oracle's AL sweep, the
bit property, what must not move, the degenerate rows, the execution tools, the state machine and the penalty helper.  The cooperative sweeps
and the batch solvers exist on the device only: tests/test_gpu_gains_al.py.

    python tests/tools/hostsim/gains_al_checks.py <libilqr_hostsim.so>
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
from tests import gains_al as ga  # noqa: E402


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    stats, rep, cov, worst = ga.new_stats(), cl.new_stats(), cc.new_stats(), dict(con_max=0.0, con_var=0.0)
    ga.check_final_penalty(ga.final_penalty)
    for case in ga.CASES:
        for T in ga.HORIZONS:
            cfg, desc, inp, systems = ga.make_case(ctx, case, T)
            pens = ga.penalties(cfg)
            p = workloads.load_batch(ctx, desc, inp, ga.B)
            try:
                for source in ("zero", "al"):
                    ga.restore(p, inp)
                    tag = f"{case} T={T} {source}"
                    plan = ga.check_plan_gains(p, cfg, inp, systems, source, pens, tag, stats)
                    if source == "al":   # the gains of the final penalty about the plan of the solve that ended with it
                        ga.check_execution(ctx, p, cfg, desc, inp, systems, plan, case, tag, rep, cov, worst)
                lam, U = ga.multipliers_and_controls(p, cfg, inp)
                for pen in pens:
                    ga.check_bits(p, inp, lam, U, pen, f"{case} T={T} bits pen={pen:.6g}")
                ga.check_degenerate(p, cfg, inp, U, f"{case} T={T}")
                if T >= 9:
                    ga.check_rows_matter(p, cfg, inp, lam, U, pens[1], f"{case} T={T}")
                    ga.check_penalty_of_last_update(p, cfg, inp, f"{case} T={T}")
            finally:
                p.close()
            print(f"{case} T={T}: oracle, unmoved, bits, degenerate rows ok", flush=True)
    ga.check_reg_case(ctx, stats)
    print(f"{ga.REG_CASE}: oracle with the same reg, unmoved, bits ok", flush=True)
    ga.check_state_machine(ctx, batch_solvers=False)
    print(f"{stats['n']} instances against the oracle's AL sweep, {stats['ill']} by its sensitivity (worst ratio {stats['worst_ratio']:.2f}), "
          f"{stats['skipped']} skipped at a mask margin below {ga.MARGIN:g}; worst share of the tolerance: K {stats['worst_K']:.3f}, d {stats['worst_d']:.3f}; "
          f"replay: {rep['n']} samples, {rep['ill']} by their sensitivity; covariance: {cov['n']} outputs, {cov['ill']} by their sensitivity; "
          f"con_max at most {worst['con_max']:.3e} of its bound, con_var at most {worst['con_var']:.3e} relative", flush=True)
    ctx.close()
    print("gains_al: ok")


if __name__ == "__main__":
    main()
