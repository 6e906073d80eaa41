"""Obstacle terms of the stage cost on the device (ilqr_problem_set_obstacles, ilqr_problem_obstacle_terms): k_obs_derivs, k_obs_query and the OBS
forms of k_init_rollout / k_backward / k_forward held to the checks of tests/obstacles.py, the _dev forms on torch tensors.  Beyond the host build's
cases: after clear_obstacles() the planned (cooperative) kernels give the bytes of a problem that never had the terms, and a multi-start group
whose starts are all blocked without the term has an eligible winner with it.  The host build: tests/test_obstacles_cpu.py."""
import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads
from tests import multistart as ms
from tests import obstacles as ob
from tests.test_gpu_multistart import TorchArrays

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


@pytest.mark.parametrize("name", list(ob.CASES))
def test_terms_against_the_reference(ctx, arrays, name):
    worst = ob.check_terms(ctx, arrays, name)
    print(f"device: {name}: worst ratio to the tolerance {worst:.3e}")


@pytest.mark.parametrize("cname,system,T,B", [("panda", "po1", 9, 70), ("gen4", "pot2", 3, 5)])
def test_terms_that_never_act(ctx, cname, system, T, B):
    ob.check_inert(ctx, cname, system, T, B, f"inert {cname} {system}")


@pytest.mark.parametrize("cname,system,T,B,al,nit", ob.ITER_CASES)
def test_iterations_against_the_restatement(ctx, cname, system, T, B, al, nit):
    with ob.generic_pin(False):   # whatever the pins say, the problem runs on the generic kernels
        ob.check_iterations(ctx, cname, system, T, B, al, nit, f"iterations {cname} {system} T={T} al={al} nit={nit}")


def test_the_term_bites(ctx):
    ob.check_bites(ctx)


@pytest.mark.parametrize("cname,system,T,B,al", [("panda", "po1", 9, 70, False), ("gen4", "pot2", 3, 5, False), ("panda", "po1", 9, 13, True),
                                                 ("gen7", "po2", 3, 5, True)])
def test_gains_about_an_obstacle_plan(ctx, cname, system, T, B, al):
    ob.check_gains(ctx, cname, system, T, B, al, f"gains {cname} {system} al={al}")


def test_nothing_else_moves(ctx, arrays):
    ob.check_untouched(ctx, arrays)


def test_refusals(ctx, arrays):
    ob.check_refusals(ctx, arrays)


def test_a_blocked_group_gets_a_winner(ctx):
    """The scenario of check (d) as a multi-start group: every start of the group runs into the obstacle without the term (no candidate: the
    group keeps member 0 and reports a clearance below the margin); with the term on the starts problem (traj_per_set = S) the coarse solves
    steer clear and the selection has eligible candidates."""
    sc, avoid = ob.check_bites_reference(ctx)
    cfg, desc, inp, chain, s, x0, sph, obs, free = sc
    S, margin, nit = 4, ob.BITE["margin"] / 2, ob.BITE["nit"]
    rb = capi.clr_robot(sph)
    tasks = workloads.load_batch(ctx, desc, inp, 1)
    starts = capi.BatchProblem(ctx, desc, S)
    try:
        for with_term in (False, True):
            starts.adopt(tasks, np.zeros(S, dtype=np.int32), capi.ADOPT_STATE | capi.ADOPT_TARGETS | capi.ADOPT_CONTROLS0)
            starts.spread_controls(S, 4711, ms.sigma_u(7, 1e-3))
            if with_term:
                starts.set_obstacles(sph, [], obs, ob.BITE["margin"], ob.BITE["weight"], S)
            starts.solve_recursive(nit, True, False)
            c = starts.clearance(rb, obs, S, margin, want=("clr_min", "eligible"))
            sel = starts.select(S, None, c.eligible)
            if with_term:
                assert sel.n_candidates[0] >= 1 and c.clr_min[sel.winner[0]] >= margin, f"with the term: {c.clr_min}"
            else:
                assert sel.n_candidates[0] == 0 and sel.winner[0] == 0 and np.all(c.clr_min < 0), f"without the term: {c.clr_min}"
    finally:
        tasks.close()
        starts.close()


# ---- the class level (PyLQR): the options of solve_batch and solve_multistart are the C-ABI sequence

def _same(got, ref, what, fields=("X", "U", "cost", "alpha", "iters", "status")):
    for f in fields:
        g = np.asarray(getattr(got, f))
        assert g.tobytes() == ref[f].astype(g.dtype).tobytes(), f"{what}: {f} differs from the sequence through capi.py"


@pytest.mark.parametrize("al", [False, True])
def test_pylqr_obstacle_options(ctx, al):
    from tests import clearance as clr
    from tests.test_gpu_multistart import _pylqr_solver

    T, G, S, seed, coarse, nit, margin, weight = 9, 5, 4, 4711, 2, 3, 0.05, 30.0
    cfg, desc, inp = ms.make_case(ctx, "C3", T, G)
    if not al:
        cfg = {k: v for k, v in cfg.items() if k != "al"}
        inp = {k: v for k, v in inp.items() if k not in ("A", "b", "lambda0")}
    a = cfg.get("al")
    sigma = ms.sigma_u(7, 0.3)
    pre = (inp["U0"], nit, a["lag"], a["penalty"], a["scaling"], True, False) if al else (inp["U0"], nit, True, False)
    sph, pl, obs = clr.multistart_world(G, np.random.default_rng(21))
    rb = capi.clr_robot(sph, pl)
    world = dict(spheres=sph, planes=pl, obstacles=obs, margin=margin)
    common = dict(S=S, seed=seed, sigma_u=sigma, coarse_iter=coarse, q0=inp["q0"], kp_targets=list(inp["targets"]))
    solver = lambda: _pylqr_solver(cfg, inp, T, al)   # noqa: E731

    # solve_batch with the options: set_obstacles (one set per instance), then the solve
    got = solver().solve_batch(*pre, q0=inp["q0"], kp_targets=list(inp["targets"]), obstacle_weight=weight, **world)
    p = workloads.load_batch(ctx, desc, inp, G)
    try:
        p.set_obstacles(sph, pl, obs, margin, weight, 1)
        ms.solve(p, cfg, nit)
        ref = dict(X=p.X(), U=p.U(), cost=p.cost(), alpha=p.alpha(), iters=p.iters(), status=p.status())
        assert np.any(p.obstacle_terms(want=("cost",)).cost > 0), "no pair is active at the plans"
    finally:
        p.close()
    _same(got, ref, "solve_batch with obstacle terms")
    plain = solver().solve_batch(*pre, q0=inp["q0"], kp_targets=list(inp["targets"]))
    zero = solver().solve_batch(*pre, q0=inp["q0"], kp_targets=list(inp["targets"]), obstacle_weight=0.0, **world)
    _same(zero, {f: np.asarray(getattr(plain, f)) for f in ("X", "U", "cost", "alpha", "iters", "status")}, "solve_batch with obstacle_weight = 0")
    assert np.asarray(plain.U).tobytes() != np.asarray(got.U).tobytes(), "the terms change nothing"

    # solve_multistart: weight 0 is the call without it; a weight puts the terms on the starts (traj_per_set = S) and on the tasks (1)
    without = solver().solve_multistart(*pre, **common, **world)
    zero = solver().solve_multistart(*pre, **common, obstacle_weight=0.0, **world)
    for f in ("X", "U", "cost", "winner", "n_candidates", "clearance", "coarse_clearance"):
        assert np.asarray(getattr(zero, f)).tobytes() == np.asarray(getattr(without, f)).tobytes(), f"solve_multistart with obstacle_weight = 0: {f}"
    got = solver().solve_multistart(*pre, **common, obstacle_weight=weight, **world)
    B = G * S
    tasks = workloads.load_batch(ctx, desc, inp, G)
    starts = capi.BatchProblem(ctx, desc, B)
    try:
        if al:
            starts.set_constraints(inp["A"], inp["b"], np.repeat(inp["lambda0"], S, axis=0))
        starts.adopt(tasks, np.arange(B) // S, capi.ADOPT_STATE | capi.ADOPT_TARGETS | capi.ADOPT_CONTROLS0)
        starts.spread_controls(S, seed, sigma)
        starts.set_obstacles(sph, pl, obs, margin, weight, S)
        tasks.set_obstacles(sph, pl, obs, margin, weight, 1)
        ms.solve(starts, cfg, coarse)
        c = starts.clearance(rb, obs, S, margin, want=("clr_min", "eligible"))
        sel = starts.select(S, None, c.eligible)
        tasks.adopt(starts, sel.winner, capi.ADOPT_CONTROLS | (capi.ADOPT_MULTIPLIERS if al else 0))
        ms.solve(tasks, cfg, nit, ms.final_penalty(coarse, a["lag"], a["penalty"], a["scaling"]) if al else None)
        ref = dict(X=tasks.X(), U=tasks.U(), cost=tasks.cost(), alpha=tasks.alpha(), iters=tasks.iters(), status=tasks.status())
        fin = tasks.clearance(rb, obs, 1, margin, want=("clr_min",))
    finally:
        tasks.close()
        starts.close()
    _same(got, ref, "solve_multistart with obstacle terms")
    assert np.array_equal(got.winner, sel.winner) and np.array_equal(got.n_candidates, sel.n_candidates)
    assert got.clearance.tobytes() == fin.clr_min.tobytes() and got.coarse_clearance.tobytes() == c.clr_min[sel.winner].tobytes()
    with pytest.raises(RuntimeError, match="obstacle_weight needs the robot's spheres"):
        solver().solve_multistart(*pre, **common, obstacle_weight=weight)
    with pytest.raises(RuntimeError, match="obstacle_weight must be finite and >= 0"):
        solver().solve_batch(*pre, q0=inp["q0"], kp_targets=list(inp["targets"]), obstacle_weight=-1.0, **world)
