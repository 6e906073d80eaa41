"""Gains about a held plan (ilqr_problem_gains) -- cases and checks shared by tests/tools/hostsim/gains_checks.py (the host build of the generic
kernels) and tests/test_gpu_gains.py (the device kernels).

(a) Oracle.  The device's own U (get_U) goes to the oracle's one-iteration ILQRRecursive solve with the line search off: its K, d are the backward
    pass about rollout(U).  Tolerances of test_gains_and_fx_outputs: K rtol 1e-6 / atol 1e-7, d rtol 1e-6 / atol 1e-9.  An entry that misses them
    may rest on the oracle's own sensitivity instead: at most ILL_FACTOR x the spread of that entry over the oracle's neutral arithmetic variants
    and over one-ulp perturbations of U (tests/parity_proof.py: VARIANTS, PERTURB), for at most one instance in ten of a case.
    Measured on the host build of the generic kernels (tests/tools/hostsim/gains_checks.py: 1256 instances over every shape, horizon and plan
    source): no instance needs that rule; the worst deviation is 0.349 of the tolerance for K and 0.026 of it for d.  On the device (one visit of
    tests/test_gpu_gains.py, the planned sweeps, every plan source): none either; 0.311 of the tolerance for K, 0.044 for d.
(b) Bits.  set_controls(U); solve_recursive(0); gains() against a fresh set_controls(U); solve_recursive(1): K byte for byte, d_solve == alpha d_gains.
(c) Nothing else moved: X, U, fX, cost, iters, status, lambda and the trace are the bytes they were; alpha is all ones.
(d) Execution: track, closed_loop and closed_loop_cov run on the new gains and reproduce the plan / the NumPy replay / the NumPy recursion.
(e) State machine: refused without a plan, accepted after every solver, invalidated as has_gains is."""
from __future__ import annotations

import numpy as np

from ilqr_planner_amd import workloads
from tests import closed_loop as cl
from tests import closed_loop_cov as cc
from tests import narrow_chain as nc
from tests import parity_proof as pp
from tests import shared_steps as ss
from tests.helpers import oracle_system_of_instance, orc

SHAPES = ("C2", "C2nd", "C4t1", "C4", "C1j", "C1t")   # PosOrn-1/2, PosOrnTime-1/2, JointSpace, JointSpaceTime
EXTRA = ("chain3", "shared", "C2hl")                   # a 3-joint chain (mapped layouts), a shared keypoint step, a second limit set
SI_SHAPES = ("C2", "C1j")                              # the single-integrator systems (k_backward_si_dpp)
HORIZONS = (2, 3, 9, 25)
B = 13
B_WIDE = 70   # more than one wave of 16-lane groups, ragged tail
K_TOL, D_TOL = dict(rtol=1e-6, atol=1e-7), dict(rtol=1e-6, atol=1e-9)
AL = dict(row=5, bound=2.0, penalty=0.25, scaling=1.1, lag=3)   # one state row q_6 <= 2.0, as the AL workloads
# solve_recursive with early_stop = 1 on the joint-space system (linear-quadratic: two iterations reach the optimum) -- (shape, T, iterations);
# STOP_CASE's iters are asserted to hold instances that stopped early
STOP_CASE = ("C1j", 9, 6)
REFUSAL = "ilqr_problem_gains needs a plan"
# The sweeps of ilqr_problem_gains read the descriptor's reg (inside the inverse of Quu only): one case away from its default of 1e-6, where a sweep
# that put reg into the value update or dropped a reg term of a closed form is off by far more than the tolerances -- (shape, T, constants)
REG_CASE = ("C3", 25, dict(reg=1e-2))


def make_case(ctx, name, T, Bn=B):
    """tests/closed_loop.make_case at any batch size: (cfg, desc, inp, systems)."""
    if name == "chain3":
        cfg = dict(nc.narrow_cfg("C2", 3), T=T)
        desc, inp = workloads.make_batch(ctx, cfg, B=Bn, chain=nc.capi_chain(3))
        segs = nc.oracle_segs(3)
        return cfg, desc, inp, [nc.oracle_system(cfg, inp, i, segs) for i in range(Bn)]
    if name == "shared":
        cfg, desc, inp, cfg_eq, inp_eq = ss.make_case(ctx, "C2", "sum", Bn, T=T)
        return cfg, desc, inp, [oracle_system_of_instance(cfg_eq, inp_eq, i) for i in range(Bn)]
    cfg = dict(workloads.config(name), T=T, shape=name)
    if name in cl.TIME_SHAPES:   # the batch seeds of tests/closed_loop.py: the plans stay bounded
        desc, inp = workloads.make_batch(ctx, cfg, B=Bn, seed=cl.TIME_PLANS.get((name, T), (1, cl.NIT_TIME))[0])
        inp["U0"][:, :, -1] = np.sqrt(cfg["ctimes"][-1] / (T - 1))
    else:
        desc, inp = workloads.make_batch(ctx, cfg, B=Bn)
    return cfg, desc, inp, [oracle_system_of_instance(cfg, inp, i) for i in range(Bn)]


def iterations(cfg):
    """Iterations of the solve that makes the plan: cfg["nit"], or those of tests/closed_loop.py."""
    if cfg.get("nit"):
        return int(cfg["nit"])
    return cl.TIME_PLANS.get((cfg.get("shape"), cfg["T"]), (1, cl.NIT_TIME))[1] if cfg.get("ctimes") else cl.NIT


def set_al_row(p, cfg):
    """One inequality row on a joint: A [1][n_x + n_u], multipliers from the bound as the AL workloads start."""
    A = np.zeros((1, p.dims.n_x + p.dims.n_u))
    A[0, AL["row"]] = 1.0
    p.set_constraints(A, np.array([AL["bound"]]), np.full((p.B, p.T - 1, 1), AL["bound"]))


def make_plan(p, cfg, source, psi=None):
    """Leaves the plan of `source` in p: zero | rec | al | stop | cp | batch.  Returns the iteration count asked for."""
    n = iterations(cfg)
    if source == "zero":
        p.solve_recursive(0, True, False)
        return 0
    if source in ("rec", "stop"):   # the solve of tests/closed_loop.py; "stop": a case where it ends some instances early
        p.solve_recursive(n, True, True)
    elif source == "al":
        set_al_row(p, cfg)
        p.solve_al(n, AL["lag"], AL["penalty"], AL["scaling"], True, True)
    elif source == "cp":
        p.solve_batch_cp(psi, n, True)
    elif source == "batch":
        p.solve_batch(n, True)
    else:
        raise KeyError(source)
    return n


def oracle_gains(s, U, variant=0, perturb=None, constants=None):
    """K, d of the oracle's backward pass about rollout(U): its one-iteration solve with the line search off (alpha = 1: d unscaled).
    constants: the solver constants of the case's descriptor (tests/solver_constants.py), None = the defaults."""
    u = np.asarray(U, float).reshape(-1)
    if perturb is not None:
        u = u * (1.0 + np.where(np.arange(u.size) % 2 == 0, perturb[0], perturb[1]) * 2.0 ** -52)
    orc.set_variant(variant)
    try:
        r = orc.solve_recursive(s, u, 1, False, False, constants=constants)
    finally:
        orc.set_variant(0)
    return r["K"], r["d"]


def new_stats():
    return dict(n=0, ill=0, worst_K=0.0, worst_d=0.0, worst_ratio=0.0)


def check_against_oracle(systems, U, K, d, status, tag, stats, instances=None, constants=None):
    """(a) for every instance (or `instances`) whose status is not NONFINITE."""
    idx = list(range(len(systems))) if instances is None else list(instances)
    n_ill = 0
    for i in idx:
        if status[i] & 1:
            continue
        Kr, dr = oracle_gains(systems[i], U[i], constants=constants)
        assert np.all(np.isfinite(K[i])) and np.all(np.isfinite(d[i])), f"{tag}: gains of instance {i} are not finite"
        okK = np.abs(K[i] - Kr) <= K_TOL["atol"] + K_TOL["rtol"] * np.abs(Kr)
        okd = np.abs(d[i] - dr) <= D_TOL["atol"] + D_TOL["rtol"] * np.abs(dr)
        stats["n"] += 1
        stats["worst_K"] = max(stats["worst_K"], float(np.max(np.abs(K[i] - Kr) / (K_TOL["atol"] + K_TOL["rtol"] * np.abs(Kr)))))
        stats["worst_d"] = max(stats["worst_d"], float(np.max(np.abs(d[i] - dr) / (D_TOL["atol"] + D_TOL["rtol"] * np.abs(dr)))))
        if okK.all() and okd.all():
            continue
        sK, sd = np.zeros_like(Kr), np.zeros_like(dr)   # the oracle's own sensitivity, per entry
        for kw in [dict(variant=v) for v in pp.VARIANTS] + [dict(perturb=pt) for pt in pp.PERTURB]:
            Kv, dv = oracle_gains(systems[i], U[i], constants=constants, **kw)
            sK, sd = np.maximum(sK, np.abs(Kv - Kr)), np.maximum(sd, np.abs(dv - dr))
        for name, got, ref, ok, sens in (("K", K[i], Kr, okK, sK), ("d", d[i], dr, okd, sd)):
            bad = ~ok & ~(np.abs(got - ref) <= pp.ILL_FACTOR * sens)
            if bad.any():
                j = np.unravel_index(np.argmax(np.where(bad, np.abs(got - ref), 0)), bad.shape)
                raise AssertionError(f"{tag}: {name}{j} of instance {i} is {got[j]!r}, the oracle's {ref[j]!r} (off by {abs(got[j] - ref[j]):.3e}); "
                                     f"its own variants move it by {sens[j]:.3e}")
            if (~ok).any():
                stats["worst_ratio"] = max(stats["worst_ratio"], float(np.max(np.where(~ok, np.abs(got - ref) / np.maximum(sens, 1e-300), 0))))
        n_ill += 1
    stats["ill"] += n_ill
    assert 10 * n_ill <= len(idx), f"{tag}: {n_ill} of {len(idx)} instances rest on the oracle's sensitivity (at most one in ten may)"
    return n_ill


def snapshot(p, n_iter):
    s = dict(X=p.X(), U=p.U(), fX=p.fX(), cost=p.cost(), iters=p.iters(), status=p.status())
    if p.m:
        s["lam"] = p.lam()
    if n_iter > 0:
        s["trace_cost"], s["trace_alpha"] = p.trace(n_iter)
    return s


def check_unmoved(before, after, alpha, tag):
    """(c)"""
    for k, v in before.items():
        assert v.tobytes() == after[k].tobytes(), f"{tag}: gains() changed {k}"
    assert np.array_equal(alpha, np.ones_like(alpha)), f"{tag}: alpha is not all ones after gains()"


def check_plan_gains(p, cfg, systems, source, tag, stats, psi=None, instances=None, want_stopped=False, constants=None):
    """A plan of `source`, gains() about it: (a) and (c).  Returns the plan dict for the execution checks."""
    n = make_plan(p, cfg, source, psi)
    before = snapshot(p, n)
    if want_stopped:
        it = before["iters"]
        assert np.any(it < n) and np.all(it >= 1), f"{tag}: no instance stopped early (iters {it})"
    p.gains()
    K, d = p.K(), p.d()
    after = snapshot(p, n)
    check_unmoved(before, after, p.alpha(), tag)
    check_against_oracle(systems, before["U"], K, d, before["status"], tag, stats, instances, constants)
    return dict(X=before["X"], U=before["U"], K=K, d=d, cost=before["cost"])


def with_constants(desc, constants):
    """A copy of the descriptor with the solver constants set (the made cases are shared: theirs stay as they are)."""
    out = type(desc).from_buffer_copy(desc)
    for k, v in constants.items():
        setattr(out, k, float(v))
    return out


def reg_moves_the_gains(Kd_at, Kd_default):
    """The condition that keeps a reg case from being vacuous, on the oracle alone: K about the same controls moves by more than 100 x its
    tolerance somewhere when reg does."""
    (K1, _), (K0, _) = Kd_at, Kd_default
    return bool(np.max(np.abs(K1 - K0) / (K_TOL["atol"] + K_TOL["rtol"] * np.abs(K0))) > 100)


def check_reg_case(ctx, stats):
    """REG_CASE: a zero plan and a recursive plan made with reg = 1e-2, gains() about them: (a) against the oracle with the same reg, (b), (c)."""
    name, T, constants = REG_CASE
    cfg, desc, inp, systems = make_case(ctx, name, T)
    desc = with_constants(desc, constants)
    p = workloads.load_batch(ctx, desc, inp, B)
    try:
        for source in ("zero", "rec"):
            plan = check_plan_gains(p, cfg, systems, source, f"{name} T={T} {source} {constants}", stats, constants=constants)
            for i in (0, 1):
                assert reg_moves_the_gains(oracle_gains(systems[i], plan["U"][i], constants=constants), oracle_gains(systems[i], plan["U"][i])), \
                    f"{name} T={T} {source}: reg does not move the gains of instance {i}"
            p.set_controls(inp["U0"])
        check_bits(p, inp, bits_controls(inp), f"{name} T={T} {constants} bits")
    finally:
        p.close()


def check_bits(p, inp, U, tag):
    """(b): under the pins in force.  U: any control sequence [B][T-1][n_u]."""
    p.set_controls(U)
    p.solve_recursive(0, True, False)
    p.gains()
    Kg, dg, ag = p.K(), p.d(), p.alpha()
    p.set_controls(U)
    p.solve_recursive(1, True, False)
    Ks, ds, a = p.K(), p.d(), p.alpha()
    p.set_controls(inp["U0"])
    assert np.all(ag == 1.0)
    assert np.all(np.isfinite(Kg)) and np.all(np.isfinite(dg)), f"{tag}: gains are not finite"
    assert np.array_equal(Ks, Kg), f"{tag}: K of gains() differs from a one-iteration solve's by {np.abs(Ks - Kg).max():.3e}"
    assert np.array_equal(ds, a[:, None, None] * dg), f"{tag}: d of a one-iteration solve is not alpha d of gains()"
    assert np.all(np.log2(a) == np.round(np.log2(a))), f"{tag}: alpha is no power of two"


def bits_controls(inp, seed=7):
    """A control sequence that is no solver's: the case's own start moved by noise of a hundredth of its size (of 1e-2 where it is zero)."""
    rng = np.random.default_rng(seed)
    U0 = inp["U0"]
    return U0 + 1e-2 * np.where(U0 != 0, np.abs(U0), 1.0) * rng.standard_normal(U0.shape)


def stage_cost_of_plan(s, X, U):
    J = sum(orc.cost(s, X[k], U[k], k) for k in range(len(U)))
    return J + orc.cost(s, X[-1], np.zeros(U.shape[1]), len(U))


def check_execution(ctx, p, cfg, desc, systems, plan, tag, cov_stats=None):
    """(d) on the plan whose gains p holds.  Returns the replay's stats (tests/closed_loop.py)."""
    X, U = plan["X"], plan["U"]
    T = X.shape[1]
    for k in range(T - 1):   # at the plan's own state the feedback term vanishes
        ut = p.track(k, X[:, k], False)
        assert cl._within(ut, U[:, k]), f"{tag}: track({k}, X[:, {k}]) leaves U[:, {k}] by {np.abs(ut - U[:, k]).max():.3e}"
    cost, Xc, Uc = p.closed_loop(samples=2)
    for s in range(2):
        assert cl._within(Xc[:, s], X), f"{tag}: the undisturbed closed loop leaves the plan by {np.abs(Xc[:, s] - X).max():.3e}"
        assert cl._within(Uc[:, s], U), tag
    J = np.array([stage_cost_of_plan(systems[b], X[b], U[b]) for b in range(len(systems))])
    np.testing.assert_allclose(cost[:, 0], J, rtol=1e-9, atol=0, err_msg=f"{tag}: J of the undisturbed closed loop is not the plan's stage cost")
    assert np.array_equal(cost[:, 0], cost[:, 1])
    st = cl.new_stats()
    x0, w = cl.perturbations(plan, 3, seed=100 + T)
    # The feed-forward of gains() is the whole Newton step d_k from the plan, not alpha d_k.  On the time systems (dt = u_last^2) the plans of a few
    # iterations are far from converged (|d| of 15 .. 55 against controls of size 1: measured on the host build) and a loop that adds that step at
    # every k leaves every bound within a few steps, in the NumPy replay as on the device: there the replay is compared without it.
    for ff in ((False,) if cfg.get("ctimes") else (False, True)):
        c, Xw, Uw = p.closed_loop(x0, w, with_feedforward=ff)
        assert np.all(np.isfinite(c)) and np.all(np.isfinite(Xw)) and np.all(np.isfinite(Uw)), f"{tag}: non-finite closed loop"
        cl.check_against_replay(systems, plan, x0, w, ff, c, Xw, Uw, f"{tag} ff={ff}", st)
    sw, sx = cc.sigmas(X.shape[2])
    cc.check_against_recursion(ctx, cfg, desc, plan, sw, sx, cc.call(p, sw, sx), tag, cov_stats if cov_stats is not None else cc.new_stats())
    return st


def refused(call, text=REFUSAL):
    cl._refused(call, text)


def check_state_machine(ctx, batch_solvers, psi_of=None):
    """(e).  batch_solvers: the build has ilqr_solve_batch_cp / ilqr_solve_batch."""
    cfg, desc, inp, _ = make_case(ctx, "C2", 9)
    p = workloads.load_batch(ctx, desc, inp, B)
    try:
        refused(p.gains)                                         # nothing solved yet
        cl._refused(p.gains, "ilqr_solve_recursive with nb_iter = 0 rolls out the controls as they are")   # the text names the remedy
        p.solve_recursive(0, True, False)
        cl._refused(lambda: p.closed_loop(samples=1), "closed loop needs the gains")
        p.gains()                                                # accepted after a 0-iteration solve
        p.closed_loop(samples=1)
        setters = (lambda: p.set_init_state(inp["q0"], inp["dq0"]), lambda: p.set_keypoint_targets(0, inp["targets"][0]), lambda: p.set_controls(inp["U0"]),
                   lambda: set_al_row(p, cfg), lambda: p.reset_multipliers(), lambda: p.warm_start(0))
        for setter in setters:
            p.solve_recursive(1, True, False)
            p.gains()
            setter()
            refused(p.gains)
            cl._refused(lambda: p.closed_loop(samples=1), "closed loop needs the gains")
        p.solve_recursive(2, True, True)
        p.gains()
        p.solve_al(2, AL["lag"], AL["penalty"], AL["scaling"], True, True)
        p.gains()
        p.closed_loop_cov(1e-3)
        if batch_solvers:
            psi = psi_of(dict(kind="unitstep", K=2), cfg["T"], p.dims.n_u)
            for solve in (lambda: p.solve_batch_cp(psi, 2, True), lambda: p.solve_batch(2, True)):
                p.gains()
                p.closed_loop(samples=1)
                solve()
                cl._refused(lambda: p.closed_loop(samples=1), "closed loop needs the gains")   # a batch solve after a gains() leaves no gains again
                cl._refused(lambda: p.closed_loop_cov(1e-3), "closed loop needs the gains")
                p.gains()                                        # ... and is a plan
                p.closed_loop(samples=1)
        ctx.synchronize()
    finally:
        p.close()
