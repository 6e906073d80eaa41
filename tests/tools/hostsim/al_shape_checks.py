"""AL-iLQR with 4 .. 32 constraint rows through the C ABI on the host build of the lane-per-instance kernels (tests/test_al_shapes_cpu.py builds the
library and runs this script in a child process of its own).  Every case of tests/al_shapes.host_cases is gated by al_shapes.check_case: the rows
bind on the oracle's solve, the parity proof with every multiplier update recomputed (tests/parity_proof.check_multipliers), gains at every step,
trajectories and final multipliers against the oracle's.  Around the solves: the multipliers in [B][T-1][m] order, reset_multipliers, and
set_constraints with another m and another per_step on a live problem.

    python tests/tools/hostsim/al_shape_checks.py <libilqr_hostsim.so>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ilqr_planner_amd import capi, workloads  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every solve of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import al_shapes as al  # noqa: E402
from tests import parity_proof as pp  # noqa: E402


def _results(p):
    return dict(cost=p.cost(), U=p.U(), X=p.X(), iters=p.iters(), lam=p.lam())


def _fresh(ctx, cfg, desc, inp):
    p = workloads.load_batch(ctx, desc, inp, len(inp["q0"]))
    try:
        workloads.run_solver(p, cfg, nb_iter=al.NIT, early_stop=True)
        return _results(p)
    finally:
        p.close()


def check_orchestration(ctx):
    """One live problem through three constraint sets: 4 shared rows, 17 dense rows per step, 4 shared rows again."""
    T = 9
    cfg, desc, inp = al.make_case(ctx, "C3", T, 4, "state")
    cfg17, _, inp17 = al.make_case(ctx, "C3", T, 17, "dense", per_step=True)
    Bn, alc = len(inp["q0"]), cfg["al"]
    want4, want17 = _fresh(ctx, cfg, desc, inp), _fresh(ctx, cfg17, desc, inp17)
    p = workloads.load_batch(ctx, desc, inp, Bn)
    try:
        # every multiplier its own value: what comes back, and what one update makes of it, is in [B][T-1][m] order
        lam0 = 1e-2 + 1e-6 * np.arange(Bn * (T - 1) * 4, dtype=float).reshape(Bn, T - 1, 4)
        p.set_constraints(inp["A"], inp["b"], lam0)
        np.testing.assert_array_equal(p.lam(), lam0)
        p.solve_al(2, alc["lag"], alc["penalty"], alc["scaling"], True, False)
        lam, X, U = p.lam(), p.X(), p.U()
        assert lam.shape == (Bn, T - 1, 4)
        for i in range(Bn):
            v, tol = pp.multiplier_update(lam0[i], X[i], U[i], inp["A"], inp["b"], pp.al_penalty(alc, 1))
            assert np.all(np.abs(lam[i] - np.maximum(v, 0)) <= tol), f"multipliers of instance {i} after one update"
        assert np.any(lam != lam0)
        p.reset_multipliers()
        np.testing.assert_array_equal(p.lam(), lam0)
        # another m and one set per step on the live problem: the solve is that of a problem that never had other rows
        for cfg_n, inp_n, want in ((cfg17, inp17, want17), (cfg, inp, want4), (cfg17, inp17, want17)):
            p.set_controls(inp_n["U0"])
            p.set_constraints(inp_n["A"], inp_n["b"], inp_n["lambda0"])
            assert p.lam().shape == inp_n["lambda0"].shape and not np.any(p.lam())
            workloads.run_solver(p, cfg_n, nb_iter=al.NIT, early_stop=True)
            got = _results(p)
            for k in want:
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} after set_constraints with m = {inp_n['lambda0'].shape[2]} on a live problem")
            p.reset_multipliers()
            assert not np.any(p.lam())
    finally:
        p.close()


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    for c in al.host_cases():
        cfg, desc, inp = al.make(ctx, c)
        print(al.check_case(ctx, cfg, desc, inp, al.case_id(c)), flush=True)
    check_orchestration(ctx)
    print("set_constraints with another m and per_step on a live problem, reset_multipliers, multipliers in [B][T-1][m] order", flush=True)
    ctx.close()
    print("al shapes: ok")


if __name__ == "__main__":
    main()
