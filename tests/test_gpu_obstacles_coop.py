"""Obstacle terms on the cooperative kernels (ilqr_ctx_set_obstacle_path(COOPERATIVE)): k_stage_dense, k_backward_si_dpp<.., SW_DENSE>, k_obs_ls and
k_obs_ls_sum held to the float64 restatement of tests/obstacle_reference.py and to the generic mode of the same library (tests/obstacles_coop.py,
and the helpers of tests/obstacles.py on a context with the mode on).  Every test needs the new symbol: none passes without it."""
import contextlib
import os

import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads
from tests import clearance as clr
from tests import multistart as ms
from tests import obstacle_reference as ref
from tests import obstacles as ob
from tests import obstacles_coop as oc
from tests.gains import D_TOL, K_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    """A context in cooperative mode; a test that switches the mode puts it back."""
    import torch

    torch.cuda.init()
    c = capi.Context(0)
    c.set_obstacle_path("cooperative")
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain_ctx():
    """A context that never heard of the mode."""
    c = capi.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------ 1. iterations against the restatement

ITER = [(c, s, al, nit) for c, s in (("panda", "po1"), ("gen7", "po1"), ("panda", "js1")) for al in (False, True) for nit in (1, 3)] + \
       [("gen4", "po1", False, 1), ("gen4", "po1", False, 3)]   # (a state row of AL_ROW's index does not exist on four joints)
ALPHAS = {}


@pytest.mark.parametrize("cname,system,al,nit", ITER)
def test_iterations_against_the_restatement(ctx, cname, system, al, nit):
    out = oc.iterations(ctx, cname, system, 9, 3, al, nit, f"coop iterations {cname} {system} al={al} nit={nit}")
    ALPHAS[(cname, system, al, nit)] = [r["alphas"] for r in out]


def test_a_step_size_below_one_decides(ctx):
    """On the restatement alone: over the cases above some accepted step size is below 1, so the per-step-size costs beyond index 0 decide."""
    if not ALPHAS:   # run on its own
        test_iterations_against_the_restatement(ctx, *ITER[1])
    below = [(k, a) for k, v in ALPHAS.items() for a in v if min(a) < 1.0]
    print(f"cases with an accepted step size below 1: {below}")
    assert below, f"every accepted step size of the restatement is 1: {ALPHAS}"


# ------------------------------------------------------------------------------------------------ 2. the dense sweep's shapes

#        T, B, traj_per_set (None: B), spheres, obstacles, planes, uniform R, AL state rows
SWEEP = [(2, 1, 1, 1, 1, 0, True, None),
         (3, 5, 5, 5, 9, 2, False, None),
         (9, 70, 1, 32, 9, 2, True, None),
         (10, 5, 1, 5, 9, 0, True, [5]),
         (17, 70, 5, 5, 9, 2, False, [5]),
         (33, 5, None, 5, 9, 2, True, [1, 3, 5, 6]),
         (9, 70, None, 1, 1, 2, False, [1, 3, 5, 6]),
         (10, 1, 1, 32, 9, 2, False, None),
         (17, 5, 5, 5, 1, 0, True, None),
         (33, 70, 5, 5, 9, 2, True, [5]),
         (2, 70, None, 5, 9, 2, False, [5]),
         (3, 1, 1, 5, 9, 2, True, [1, 3, 5, 6])]


@pytest.mark.parametrize("T,B,tps,n_sph,n_obs,n_pl,uniform,rows", SWEEP)
def test_dense_sweep_against_generic_mode(ctx, T, B, tps, n_sph, n_obs, n_pl, uniform, rows):
    oc.check_sweep(ctx, T, B, tps, n_sph, n_obs, n_pl, uniform, rows, f"sweep T={T} B={B} tps={tps} sph={n_sph} obs={n_obs} planes={n_pl} unif={uniform} rows={rows}")


def test_dense_sweep_eight_lane_grouping(ctx):
    import torch

    B = 16 * torch.cuda.get_device_properties(0).multi_processor_count + 4   # 4 n_simd + 4: the first batch on 8 lanes per instance
    oc.check_sweep(ctx, 3, B, None, 5, 9, 2, True, [5], f"sweep T=3 B={B} (8 lanes)")


# ------------------------------------------------------------------------------------------------ 3. limit terms of the dense kernel

def test_limit_terms_at_steps_without_keypoint(ctx):
    T, width = 9, 0.05
    out = oc.iterations(ctx, "panda", "po1", T, 1, False, 3, "coop limits", prepare=oc.narrow_limits(width))
    cfg, desc, inp, chain = ob.make_problem(ctx, "panda", "po1", T, 1, R=ob.R_C, u_scale=0.2)
    q0 = np.asarray(inp["q0"][0][:7])
    X = np.asarray(out[0]["X"])[:, :7]
    free = [k for k in range(T) if k not in list(inp["kp_t"])]
    beyond = np.abs(X[free] - q0[None, :]) > width
    print(f"limits: steps without keypoint {free}: {int(beyond.sum())} (step, joint) pairs beyond a limit")
    assert beyond.any(), "no joint of the restated plan is beyond its limit at a step without keypoint: the case shows nothing"


# ------------------------------------------------------------------------------------------------ 4. cost of a 0-iteration solve

@pytest.mark.parametrize("T,B", [(9, 5), (33, 70)])
def test_initial_cost_against_generic_mode(ctx, T, B):
    cfg, desc, inp, chain = ob.make_problem(ctx, "panda", "po1", T, B, R=ob.R_C, u_scale=0.2)
    sph, pl, obs = ob.iter_world(chain, inp, 31 + T)
    p = workloads.load_batch(ctx, desc, inp, B)
    try:
        p.set_obstacles(sph, pl, obs, ob.MARGIN, 20.0, 1)
        p.solve_recursive(0, True, False)
        c1, t1, X1 = p.cost(), p.obstacle_terms(), p.X()
        oc.coop(ctx, False)
        p.solve_recursive(0, True, False)
        c0, t0 = p.cost(), p.obstacle_terms()
        assert X1.tobytes() == p.X().tobytes()
        assert np.any(t0.cost > 0)
        rel = np.abs(c1 - c0) / c0
        print(f"initial cost T={T} B={B}: worst |difference| / cost {rel.max():.3e} (bound {4 * T * 2.0 ** -53:.3e})")
        assert np.all(np.abs(c1 - c0) <= 4 * T * 2.0 ** -53 * c0)
        for f in ("cost", "lx", "lxx"):
            assert getattr(t1, f).tobytes() == getattr(t0, f).tobytes(), f"obstacle_terms: {f} differs between the modes"
    finally:
        oc.coop(ctx, True)
        p.close()


# ------------------------------------------------------------------------------------------------ 5. terms that never act

@pytest.mark.parametrize("what", ["far", "weight0"])
@pytest.mark.parametrize("nit", [1, 3])
def test_inert_terms_against_the_restatement_without_a_world(ctx, what, nit):
    T, B = 9, 3
    chain = clr.chain_of("panda")
    sph = clr.spheres_of(chain, 5, np.random.default_rng(9))
    lib = (sph, [], np.repeat(ob.FAR, B, axis=0), 10.0) if what == "far" else (sph, [], clr.obstacles_of(B, 3, np.random.default_rng(10)), 0.0)
    oc.iterations(ctx, "panda", "po1", T, B, False, nit, f"coop inert {what} nit={nit}", lib_world=lib, with_ref_world=False)


def test_no_terms_no_difference(ctx, plain_ctx):
    """After clear_obstacles(), and on a problem that never had terms, the mode changes no byte."""
    T, B, nit = 9, 13, 3
    cfg, desc, inp, chain = ob.make_problem(ctx, "panda", "po1", T, B)
    sph, pl, obs = ob.iter_world(chain, inp, 3)
    p, q, r = workloads.load_batch(ctx, desc, inp, B), workloads.load_batch(plain_ctx, desc, inp, B), workloads.load_batch(ctx, desc, inp, B)
    try:
        q.solve_recursive(nit, True, False)
        want = ob.full_results(q, cfg, nit)
        p.set_obstacles(sph, pl, obs, ob.MARGIN, 20.0, 1)
        p.solve_recursive(nit, True, False)
        assert p.U().tobytes() != want["U"].tobytes(), "the terms change nothing"
        p.clear_obstacles()
        p.set_controls(inp["U0"])
        p.solve_recursive(nit, True, False)
        ms.same(want, ob.full_results(p, cfg, nit), "after clear_obstacles in cooperative mode")
        r.solve_recursive(nit, True, False)
        ms.same(want, ob.full_results(r, cfg, nit), "a problem without terms in cooperative mode")
    finally:
        for h in (p, q, r):
            h.close()


# ------------------------------------------------------------------------------------------------ 6. the generic pin wins

def test_generic_pin_wins_over_the_mode(ctx, plain_ctx):
    T, B, nit = 9, 13, 3
    cfg, desc, inp, chain = ob.make_problem(ctx, "panda", "po1", T, B, R=ob.R_C, u_scale=0.2)
    sph, pl, obs = ob.iter_world(chain, inp, 3)
    p, q = workloads.load_batch(ctx, desc, inp, B), workloads.load_batch(plain_ctx, desc, inp, B)
    try:
        for h in (p, q):
            h.set_obstacles(sph, pl, obs, ob.MARGIN, 20.0, 1)
        q.solve_recursive(nit, True, False)   # mode off, no pin: the generic set
        with ob.generic_pin():
            p.solve_recursive(nit, True, False)
        ms.same(ob.full_results(q, cfg, nit), ob.full_results(p, cfg, nit), "generic pin in cooperative mode")
    finally:
        p.close()
        q.close()


# ------------------------------------------------------------------------------------------------ 7. gains and bites

@pytest.mark.parametrize("B,al", [(70, False), (13, True)])
def test_gains_about_an_obstacle_plan(ctx, B, al):
    ob.check_gains(ctx, "panda", "po1", 9, B, al, f"coop gains al={al}")


def test_the_term_bites(ctx):
    sc, avoid = ob.check_bites_reference(ctx)
    cfg, desc, inp, chain, s, x0, sph, obs, free = sc
    rb = capi.clr_robot(sph)
    p = workloads.load_batch(ctx, desc, inp, 1)
    try:
        p.set_obstacles(sph, [], obs, ob.BITE["margin"], ob.BITE["weight"], 1)
        p.solve_recursive(ob.BITE["nit"], True, False)   # unpinned: the cooperative path
        got = p.clearance(rb, obs, 1, ob.BITE["margin"])
        print(f"bites: step sizes {list(p.trace(ob.BITE['nit'])[1][0])}, clr_min {got.clr_min[0]:.4f}")
        assert list(p.trace(ob.BITE["nit"])[1][0]) == avoid["alphas"], "step sizes against the restatement"
        assert np.allclose(p.X()[0], avoid["X"], rtol=1e-6, atol=1e-8), "the library's plan with the term is not the restated one"
        assert got.clr_min[0] >= ob.BITE["margin"] / 2, f"the library's plan with the term has clr_min {got.clr_min[0]}"
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ 8. independence

def _solve_slice(ctx, cfg, desc, inp, sph, pl, obs, n, nit, al):
    sub = dict(inp, q0=inp["q0"][:n], dq0=inp["dq0"][:n], U0=inp["U0"][:n], targets=[t[:n] for t in inp["targets"]])
    p = workloads.load_batch(ctx, desc, sub, n)
    try:
        p.set_obstacles(sph, pl, obs[:n], ob.MARGIN, 20.0, 1)
        if al:
            oc.set_al_rows(p, n, p.T, [ob.AL_ROW["row"]])
            p.solve_al(nit, 2, ob.AL_ROW["penalty"], 1.1, True, False)
        else:
            p.solve_recursive(nit, True, False)
        return ob.full_results(p, cfg, nit)
    finally:
        p.close()


@pytest.mark.parametrize("al", [False, True])
def test_an_instance_does_not_see_its_batch(ctx, al):
    T, nit = 9, 3
    cfg, desc, inp, chain = ob.make_problem(ctx, "panda", "po1", T, 70, R=ob.R_C, u_scale=0.2)
    sph, pl, obs = ob.iter_world(chain, inp, 8)
    res = {}
    for pin in ("", "wg", "wglds"):
        with env(ILQR_FWD=pin):
            big, small = _solve_slice(ctx, cfg, desc, inp, sph, pl, obs, 70, nit, al), _solve_slice(ctx, cfg, desc, inp, sph, pl, obs, 5, nit, al)
        for k, v in small.items():
            assert v.tobytes() == big[k][:5].tobytes(), f"forward pin {pin!r}: {k} of an instance depends on the batch size"
        res[pin] = big
    ms.same(res["wg"], res["wglds"], "ILQR_XC_FWD_WG against ILQR_XC_FWD_WG_LDS")
    bad = dict(inp, U0=inp["U0"].copy())
    bad["U0"][2, 1, 3] = np.nan
    got = _solve_slice(ctx, cfg, desc, bad, sph, pl, obs, 70, nit, al)
    keep = np.arange(70) != 2
    for k, v in res[""].items():
        assert got[k][keep].tobytes() == v[keep].tobytes(), f"a non-finite U0 in instance 2 moves {k} of another instance"
    assert got["status"][2] & capi.STATUS_NONFINITE if hasattr(capi, "STATUS_NONFINITE") else got["status"][2] & 1


# ------------------------------------------------------------------------------------------------ 9. refusals and bindings

def test_bad_path_values_are_refused(ctx):
    assert ctx.L.ilqr_ctx_set_obstacle_path(ctx.h, 2) != 0
    assert "ilqr_ctx_set_obstacle_path: path must be" in ctx.L.ilqr_last_error(ctx.h).decode()
    assert ctx.L.ilqr_ctx_set_obstacle_path(ctx.h, -1) != 0
    with pytest.raises(ValueError, match="set_obstacle_path"):
        ctx.set_obstacle_path("fast")
    with pytest.raises(RuntimeError, match="path must be"):
        ctx.set_obstacle_path(7)
    ctx.crosscheck_from_env()   # the pins do not touch the mode: the next test would fail on the generic set's bytes
    ctx.set_obstacle_path("cooperative")


def test_a_time_system_is_planned_as_before(ctx, plain_ctx):
    T, B, nit = 5, 5, 2
    cfg, desc, inp, chain = ob.make_problem(ctx, "gen4", "pot2", T, B, R=ob.R_C, u_scale=0.2)
    sph, pl, obs = ob.iter_world(chain, inp, 3)
    p, q = workloads.load_batch(ctx, desc, inp, B), workloads.load_batch(plain_ctx, desc, inp, B)
    try:
        for h in (p, q):
            h.set_obstacles(sph, pl, obs, ob.MARGIN, 20.0, 1)
            h.solve_recursive(nit, True, False)
        ms.same(ob.full_results(q, cfg, nit), ob.full_results(p, cfg, nit), "PosOrnTime-2 in cooperative mode")
    finally:
        p.close()
        q.close()


def test_a_blocked_group_gets_a_winner(ctx):
    """tests/test_gpu_obstacles.py's group, its coarse solves on the cooperative path."""
    sc, avoid = ob.check_bites_reference(ctx)
    cfg, desc, inp, chain, s, x0, sph, obs, free = sc
    S, margin, nit = 4, ob.BITE["margin"] / 2, ob.BITE["nit"]
    rb = capi.clr_robot(sph)
    tasks = workloads.load_batch(ctx, desc, inp, 1)
    starts = capi.BatchProblem(ctx, desc, S)
    try:
        starts.adopt(tasks, np.zeros(S, dtype=np.int32), capi.ADOPT_STATE | capi.ADOPT_TARGETS | capi.ADOPT_CONTROLS0)
        starts.spread_controls(S, 4711, ms.sigma_u(7, 1e-3))
        starts.set_obstacles(sph, [], obs, ob.BITE["margin"], ob.BITE["weight"], S)
        starts.solve_recursive(nit, True, False)
        c = starts.clearance(rb, obs, S, margin, want=("clr_min", "eligible"))
        sel = starts.select(S, None, c.eligible)
        assert sel.n_candidates[0] >= 1 and c.clr_min[sel.winner[0]] >= margin, f"with the term: {c.clr_min}"
    finally:
        tasks.close()
        starts.close()


def _same(got, want, what, fields=("X", "U", "cost", "alpha", "iters", "status")):
    for f in fields:
        g = np.asarray(getattr(got, f))
        assert g.tobytes() == want[f].astype(g.dtype).tobytes(), f"{what}: {f} differs from the sequence through capi.py"


@pytest.mark.parametrize("al", [False, True])
def test_pylqr_obstacle_path(ctx, al):
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
    world = dict(spheres=sph, planes=pl, obstacles=obs, margin=margin, obstacle_weight=weight)
    common = dict(S=S, seed=seed, sigma_u=sigma, coarse_iter=coarse, q0=inp["q0"], kp_targets=list(inp["targets"]))
    solver = lambda: _pylqr_solver(cfg, inp, T, al)   # noqa: E731
    fields = ("X", "U", "cost", "alpha", "iters", "status")

    got = solver().solve_batch(*pre, q0=inp["q0"], kp_targets=list(inp["targets"]), obstacle_path="cooperative", **world)
    p = workloads.load_batch(ctx, desc, inp, G)
    try:
        p.set_obstacles(sph, pl, obs, margin, weight, 1)
        ms.solve(p, cfg, nit)
        want = dict(X=p.X(), U=p.U(), cost=p.cost(), alpha=p.alpha(), iters=p.iters(), status=p.status())
    finally:
        p.close()
    _same(got, want, "solve_batch, obstacle_path = cooperative")
    # the mode is the call's: the next call without it is today's, and "generic" is the call without the option
    plain = solver().solve_batch(*pre, q0=inp["q0"], kp_targets=list(inp["targets"]), **world)
    named = solver().solve_batch(*pre, q0=inp["q0"], kp_targets=list(inp["targets"]), obstacle_path="generic", **world)
    _same(named, {f: np.asarray(getattr(plain, f)) for f in fields}, "solve_batch, obstacle_path = generic")
    assert np.asarray(plain.X).tobytes() != np.asarray(got.X).tobytes() or np.asarray(plain.cost).tobytes() != np.asarray(got.cost).tobytes(), \
        "the two paths give the same bytes: the option did nothing, or the mode was not restored"
    with pytest.raises(RuntimeError, match="obstacle_path must be"):
        solver().solve_batch(*pre, q0=inp["q0"], kp_targets=list(inp["targets"]), obstacle_path="fast", **world)

    got = solver().solve_multistart(*pre, **common, obstacle_path="cooperative", **world)
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
        want = dict(X=tasks.X(), U=tasks.U(), cost=tasks.cost(), alpha=tasks.alpha(), iters=tasks.iters(), status=tasks.status())
    finally:
        tasks.close()
        starts.close()
    _same(got, want, "solve_multistart, obstacle_path = cooperative")
    assert np.array_equal(got.winner, sel.winner) and np.array_equal(got.n_candidates, sel.n_candidates)
    with pytest.raises(RuntimeError, match="obstacle_path must be"):
        solver().solve_multistart(*pre, **common, obstacle_path="", **world)
