"""Clearance of plans and executions on the device (ilqr_problem_clearance, ilqr_clearance_trajectories): k_clr_plan, k_clr_traj, k_clr_fold and
k_clr_stats held to the checks of tests/clearance.py, the _dev forms on torch tensors.  Beyond the host build's cases: the plan of C4 at
B = 2048 under AUTO, left by two halves on two streams, and the class level: solve_multistart of PyLQR with and without obstacles against the same
sequence through capi.py, PyLQR.clearance against Context.clearance_trajectories.  The host build: tests/test_clearance_cpu.py."""
import numpy as np
import pytest

from ilqr_planner_amd import capi
from tests import clearance as clr
from tests import multistart as ms
from tests.test_gpu_multistart import TorchArrays, _pylqr_solver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch

    torch.cuda.init()  # torch's device first, then the library's context (the _dev forms are handed torch tensors)
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def arrays():
    return TorchArrays()


@pytest.mark.parametrize("name", list(clr.CASES))
def test_against_the_reference(ctx, arrays, name):
    clr.check_reference(ctx, arrays, name)


def test_exact_ties(ctx, arrays):
    clr.check_ties(ctx, arrays)


def test_exact_boundary(ctx, arrays):
    clr.check_boundary(ctx, arrays)


def test_bad_steps(ctx, arrays):
    clr.check_bad_steps(ctx, arrays)


@pytest.mark.parametrize("cname,system,T,B,tps", clr.FORMS)
def test_problem_form_is_the_trajectory_form(ctx, arrays, cname, system, T, B, tps):
    clr.check_forms(ctx, arrays, cname, system, T, B, tps, f"{cname} {system} T={T} B={B}")


def test_plan_left_by_two_halves(ctx, arrays):
    clr.check_split_plan(ctx, arrays)


def test_executions_against_the_reference(ctx, arrays):
    clr.check_executions(ctx, arrays)


def test_selection_takes_the_cheapest_clear_member(ctx, arrays):
    clr.check_selection(ctx, arrays)


def test_nothing_else_moves(ctx, arrays):
    clr.check_untouched(ctx, arrays)


def test_refusals(ctx, arrays):
    clr.check_refusals(ctx, arrays)


# ---- (i) the class level

@pytest.mark.parametrize("al", [False, True])
def test_solve_multistart_with_and_without_obstacles(ctx, al):
    T, G, S, seed, coarse, nit, margin = 9, 5, 6, 4711, 2, 3, 0.02
    cfg, desc, inp = ms.make_case(ctx, "C3", T, G)
    if not al:
        cfg = {k: v for k, v in cfg.items() if k != "al"}
        inp = {k: v for k, v in inp.items() if k not in ("A", "b", "lambda0")}
    sigma = ms.sigma_u(7, 0.3)
    a = cfg.get("al")
    pre = (inp["U0"], nit, a["lag"], a["penalty"], a["scaling"], True, False) if al else (inp["U0"], nit, True, False)
    common = dict(S=S, seed=seed, sigma_u=sigma, coarse_iter=coarse, q0=inp["q0"], kp_targets=list(inp["targets"]))
    kept = ("X", "U", "cost", "alpha", "iters", "status")

    def same(got, ref, what):
        for f in kept:
            assert np.asarray(getattr(got, f)).tobytes() == ref[f].astype(np.asarray(getattr(got, f)).dtype).tobytes(), f"{what}: {f} differs from the sequence by hand"

    # without obstacles: what it returned before there were any
    got = _pylqr_solver(cfg, inp, T, al).solve_multistart(*pre, **common)
    ref, sel, first = ms.multistart_by_hand(ctx, cfg, desc, inp, S, seed, sigma, coarse, nit)
    same(got, ref, "solve_multistart without obstacles")
    assert np.array_equal(got.winner, sel.winner) and np.array_equal(got.n_candidates, sel.n_candidates)
    assert got.coarse_best.tobytes() == sel.best.tobytes() and got.coarse_first.tobytes() == first.tobytes()
    assert got.clearance is None and got.coarse_clearance is None and got.clearance_at is None and got.n_below is None
    # with obstacles: the same sequence with the clearance calls in it
    sph, pl, obs = clr.multistart_world(G, np.random.default_rng(21))
    got = _pylqr_solver(cfg, inp, T, al).solve_multistart(*pre, **common, spheres=sph, planes=pl, obstacles=obs, margin=margin)
    ref, sel, coarse_clr, fin = clr.multistart_by_hand(ctx, cfg, desc, inp, S, seed, sigma, coarse, nit, capi.clr_robot(sph, pl), obs, margin)
    same(got, ref, "solve_multistart with obstacles")
    assert np.array_equal(got.winner, sel.winner) and np.array_equal(got.n_candidates, sel.n_candidates)
    assert got.clearance.tobytes() == fin.clr_min.tobytes() and np.array_equal(got.clearance_at, fin.clr_at) and np.array_equal(got.n_below, fin.n_below)
    assert got.coarse_clearance.tobytes() == coarse_clr.clr_min[sel.winner].tobytes()
    elig = coarse_clr.eligible.reshape(G, S)
    assert np.any(elig == 0) and np.any(elig[:-1] == 1), f"the obstacles must exclude some starts and leave some: {elig}"
    assert np.all(coarse_clr.clr_min[sel.winner][sel.n_candidates > 0] >= margin)
    assert got.n_candidates[-1] == 0 and got.winner[-1] == (G - 1) * S and got.coarse_clearance[-1] < 0 and got.clearance[-1] < 0


def _pylqr_system(cfg, inp, T):
    """The PosOrn-1 system of tests/test_gpu_multistart._pylqr_solver: the Panda of tests/golden without a tool frame."""
    import os

    from PyLQR.sim import KDLRobot
    from PyLQR.system import PosOrnKeypoint, PosOrnPlannerSys
    from ilqr_planner_amd import workloads
    from tests.helpers import GOLDEN

    qMax = np.full(7, 10 * np.pi)
    rbt = KDLRobot(os.path.join(GOLDEN, "panda_chain.urdf"), "panda_link0", "panda_tip", list(inp["q0"][0]), [0.0] * 7)
    kps = [PosOrnKeypoint(np.array(tg[0][0:3]), np.array(tg[0][3:7]), np.diag(cfg["Qdiag"][k]), int(inp["kp_t"][k])) for k, tg in enumerate(inp["targets"])]
    return PosOrnPlannerSys(rbt, kps, list(workloads.control_weights(cfg, 7)), qMax, -qMax, T, 1, cfg["dt"])


def test_pylqr_clearance_is_the_c_abi_call(ctx):
    import os
    import sys

    from tests.helpers import ROOT

    sys.path.insert(0, os.path.join(ROOT, "ilqr_planner_amd", "pylqr"))
    import PyLQR

    T, G = 9, 5
    cfg, desc, inp = ms.make_case(ctx, "C3", T, G)
    sph, pl, obs = clr.multistart_world(G, np.random.default_rng(22))
    X = clr.states_of(G * 3, T, clr.chain_of("panda0"), "po1", np.random.default_rng(23))
    ref = ctx.clearance_trajectories(desc, X, capi.clr_robot(sph, pl), obs, 3, 0.02, stats_group=3)
    got = PyLQR.clearance(_pylqr_system(cfg, inp, T), X, sph, planes=pl, obstacles=obs, margin=0.02, traj_per_set=3, stats_group=3)
    for f in capi.Clearance._fields:
        assert np.asarray(getattr(got, f)).tobytes() == getattr(ref, f).astype(np.asarray(getattr(got, f)).dtype).tobytes(), f"PyLQR.clearance: {f}"
