"""Gains with the AL constraint terms about a held plan (ilqr_problem_gains_al) -- cases and checks shared by
tests/tools/hostsim/gains_al_checks.py (the host build of the generic kernels) and tests/test_gpu_gains_al.py (the device kernels).  The cases are
those of tests/closed_loop_con.py: the rows of tests/al_shapes.make_case on C3 (m = 1, 4 state, 5 dense), C2ndal (2, control), C4t1al (2 per
step), C4al (16) and one row on the 3-joint chain, at T = 2, 3, 9, 25 on a ragged batch of 13.

(a) Oracle.  The device's own U and multipliers (get_U, get_lambda) go to the oracle's one-iteration AL solve with lag 2 (no update in the first
    iteration), scaling 1 and the line search off: its K, d are the AL sweep about rollout(U).  Tolerances and the sensitivity rule of
    tests/gains.py (K_TOL, D_TOL, ILL_FACTOR times the spread over the oracle's arithmetic variants and one-ulp perturbations of U, at most one
    instance in ten of a case).  An instance whose probe shows mask_margin_in < 1e-9 -- a row with lambda == 0 and g at rounding distance from
    0, where the oracle's own rollout may decide the weight differently -- may be skipped, at most one in ten of a case.  It is skipped only where
    it misses the tolerances: the bounds are batch medians of a state's maximum, so the middle instance of a row sits on its bound exactly
    wherever that maximum is the start state (3 of 13 instances of C3-m4 at T = 2), and both sides decide such a row alike.
    Measured on the host build of the generic kernels (tests/tools/hostsim/gains_al_checks.py: 1456 instances over every case, horizon, plan source
    and penalty): the reference alone keeps every case within both caps -- no instance needs the sensitivity rule and none is skipped; the worst
    deviation is 0.010 of the tolerance for K and 0.007 of it for d.  On the device (one visit of tests/test_gpu_gains_al.py, the planned sweeps,
    Batch-CP plans and B = 70 included): none by the rule, none skipped; 0.019 of the tolerance for K, 0.019 for d.
(b) Bits.  set_constraints(A, b, lam) with lam of an earlier solve; set_controls(U); solve_al(0); gains_al(pen) against a fresh
    set_constraints(A, b, lam); set_controls(U); solve_al(1, 2, pen, 1.0, 1, 0): K byte for byte, d_solve == alpha d_gains.
(c) Nothing else moved: X, U, fX, cost, iters, status, lambda and the trace are the bytes they were; alpha is all ones.
(d) Degenerate rows: with bounds so far away that every row is inactive and lambda = 0, and with penalty = 0 and lambda = 0, gains_al equals
    gains() within K_TOL / D_TOL.
(e) Execution on the AL gains: tests/gains.check_execution (track, the closed loops against the NumPy replay, the covariance against the NumPy
    recursion) and closed_loop_report_con / closed_loop_cov_con against the longdouble reference of tests/closed_loop_con.py.
(f) State machine and refusals by their texts; the profile's launch counts.
(g) final_penalty is the solver's own repeated product, and the penalty of the update that ends a solve of `lag` iterations."""
from __future__ import annotations

import numpy as np

from ilqr_planner_amd import workloads
from tests import al_shapes as als
from tests import closed_loop as cl
from tests import closed_loop_con as con
from tests import gains as gn
from tests import horizons as hz
from tests import narrow_chain as nc
from tests import parity_proof as pp
from tests.helpers import oracle_system_of_instance, orc

CASES = tuple(con.CASES)
HORIZONS = gn.HORIZONS
B, B_WIDE = gn.B, gn.B_WIDE
NIT, LAG = als.NIT, als.LAG
MARGIN = 1e-9                        # (a): mask_margin_in below which an instance may be skipped
SPLIT = ("C4al-m16", 9, 2048)        # the one split case of the device tests
FAR = 1e6                            # (d): what is added to every bound
K_TOL, D_TOL = gn.K_TOL, gn.D_TOL
NO_ROWS = "ilqr_problem_gains_al needs constraint rows"
NO_PLAN = "ilqr_problem_gains_al needs a plan"
BAD_PENALTY = "the penalty must be finite and >= 0"
REG_CASE = ("C3-m1", 25, dict(reg=1e-2))   # as gains.REG_CASE, for the sweeps of ilqr_problem_gains_al

# (e): tests/closed_loop_con.py picked its sigmas for T <= 10.  At T = 25 the executions of PosOrnTime-2 about a plan of six AL iterations leave
# every bound under them (non-finite on the host build, in closed_loop_noise alone: no property of the gains under test); a hundredth keeps them finite
CON_SIGMA_SCALE = {("C4al-m16", 25): 1e-2}

_cases = {}


def final_penalty(nb_iter, lag, penalty, scaling):
    """The penalty an AL solve ends with: one `penalty *= scaling` per update iteration ((it + 1) % lag == 0, it < nb_iter), as the solver forms it."""
    pen = float(penalty)
    for it in range(int(nb_iter)):
        if (it + 1) % int(lag) == 0:
            pen *= float(scaling)
    return pen


def make_case(ctx, case, T, Bn=B):
    """(cfg, desc, inp, systems) of a case of tests/closed_loop_con.CASES; the rows and bounds are those of the batch of 13 at any batch size
    (Bn != 13: the workload's batch of that size under the same rows, multipliers zero).  Made once per (case, T, Bn)."""
    key = (case, T, Bn)
    if key in _cases:
        return _cases[key]
    name = con.CASES[case][0]
    cfg, desc, inp = con.make_case(ctx, case, T)
    if Bn != B:
        assert name != "chain3"
        A, b = inp["A"], inp["b"]
        cfg_al = cfg["al"]
        cfg, desc, inp = hz.make_case(ctx, name, T, B=Bn)
        cfg["al"] = cfg_al
        inp = dict(inp, A=A, b=b, lambda0=np.zeros((Bn, T - 1, A.shape[-2])))
    cfg = dict(cfg, al=dict(cfg["al"], lag=LAG))
    if name == "chain3":
        segs = nc.oracle_segs(3)
        systems = [nc.oracle_system(cfg, inp, i, segs) for i in range(Bn)]
    else:
        systems = [oracle_system_of_instance(cfg, inp, i) for i in range(Bn)] if Bn <= B_WIDE else None
    _cases[key] = (cfg, desc, inp, systems)
    return _cases[key]


def penalties(cfg):
    """The workload's initial penalty and the one its solve of NIT iterations ends with."""
    al = cfg["al"]
    return al["penalty"], final_penalty(NIT, al["lag"], al["penalty"], al["scaling"])


def make_plan(p, cfg, inp, source, psi=None):
    """Leaves the plan of `source` in p: zero (0-iteration solve_al) | al (NIT iterations, lag 2) | cp (Batch-CP after that solve, on its multipliers
    and from the case's own controls).  Returns the iteration count of the trace."""
    al = cfg["al"]
    if source == "zero":
        p.solve_al(0, al["lag"], al["penalty"], al["scaling"], True, False)
        return 0
    p.solve_al(NIT, al["lag"], al["penalty"], al["scaling"], True, True)
    if source == "al":
        return NIT
    assert source == "cp", source
    lam = p.lam()
    p.set_constraints(inp["A"], inp["b"], lam)
    p.set_controls(inp["U0"])
    p.solve_batch_cp(psi, cl.NIT, True)
    return cl.NIT


def restore(p, inp):
    p.set_constraints(inp["A"], inp["b"], inp["lambda0"])
    p.set_controls(inp["U0"])


# ----------------------------------------------------------------------------------------------------------- (a)

def oracle_gains(s, A, b, lam, U, pen, variant=0, perturb=None, constants=None):
    """(K, d, mask_margin_in) of the oracle's AL sweep about rollout(U) with the multipliers lam and the penalty pen.
    constants: the solver constants of the case's descriptor (tests/solver_constants.py), None = the defaults."""
    u = np.asarray(U, float).reshape(-1)
    if perturb is not None:
        u = u * (1.0 + np.where(np.arange(u.size) % 2 == 0, perturb[0], perturb[1]) * 2.0 ** -52)
    orc.set_variant(variant)
    try:
        r = orc.solve_al(s, A, b, lam, u, 1, 2, pen, 1.0, line_search=False, early_stop=False, probe=True, constants=constants)
    finally:
        orc.set_variant(0)
    return r["K"], r["d"], r["probe"][0]["mask_margin_in"]


def new_stats():
    return dict(gn.new_stats(), skipped=0)


def check_against_oracle(systems, inp, U, lam, pen, K, d, status, tag, stats, instances=None, constants=None):
    """(a) for every instance (or `instances`) whose status is not NONFINITE."""
    idx = list(range(len(systems))) if instances is None else list(instances)
    A, b = inp["A"], inp["b"]
    n_ill = n_skip = 0
    for i in idx:
        if status[i] & 1:
            continue
        Kr, dr, margin = oracle_gains(systems[i], A, b, lam[i], U[i], pen, constants=constants)
        assert np.all(np.isfinite(K[i])) and np.all(np.isfinite(d[i])), f"{tag}: gains of instance {i} are not finite"
        tK, td = K_TOL["atol"] + K_TOL["rtol"] * np.abs(Kr), D_TOL["atol"] + D_TOL["rtol"] * np.abs(dr)
        okK, okd = np.abs(K[i] - Kr) <= tK, np.abs(d[i] - dr) <= td
        if margin < MARGIN and not (okK.all() and okd.all()):   # the skip is for an instance that needs it: a row that sits ON its bound to the
            n_skip += 1                                          # last bit (x_0 of the batch's middle instance at T = 2) is decided alike by both sides
            continue
        stats["n"] += 1
        stats["worst_K"] = max(stats["worst_K"], float(np.max(np.abs(K[i] - Kr) / tK)))
        stats["worst_d"] = max(stats["worst_d"], float(np.max(np.abs(d[i] - dr) / td)))
        if okK.all() and okd.all():
            continue
        sK, sd = np.zeros_like(Kr), np.zeros_like(dr)   # the oracle's own sensitivity, per entry
        for kw in [dict(variant=v) for v in pp.VARIANTS] + [dict(perturb=pt) for pt in pp.PERTURB]:
            Kv, dv, _ = oracle_gains(systems[i], A, b, lam[i], U[i], pen, constants=constants, **kw)
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
    stats["skipped"] += n_skip
    assert 10 * n_ill <= len(idx), f"{tag}: {n_ill} of {len(idx)} instances rest on the oracle's sensitivity (at most one in ten may)"
    assert 10 * n_skip <= len(idx), f"{tag}: {n_skip} of {len(idx)} instances have a row at rounding distance from its bound (at most one in ten may be skipped)"


def check_plan_gains(p, cfg, inp, systems, source, pens, tag, stats, psi=None, instances=None, constants=None):
    """A plan of `source`, gains_al(pen) about it for every pen of `pens`: (a) and (c).  Returns the plan dict (gains of the last pen)."""
    n = make_plan(p, cfg, inp, source, psi)
    before = gn.snapshot(p, n)
    for pen in pens:
        p.gains_al(pen)
        K, d = p.K(), p.d()
        gn.check_unmoved(before, gn.snapshot(p, n), p.alpha(), f"{tag} pen={pen:.6g}")
        if systems is not None:
            check_against_oracle(systems, inp, before["U"], before["lam"], pen, K, d, before["status"], f"{tag} pen={pen:.6g}", stats, instances,
                                 constants)
    return dict(X=before["X"], U=before["U"], K=K, d=d, cost=before["cost"], lam=before["lam"], status=before["status"])


def check_reg_case(ctx, stats):
    """REG_CASE: a zero plan and an AL plan made with reg = 1e-2, gains_al about them at both penalties: (a) against the oracle with the same reg, (c);
    then (b) on the multipliers and controls of that solve."""
    case, T, constants = REG_CASE
    cfg, desc, inp, systems = make_case(ctx, case, T)
    p = workloads.load_batch(ctx, gn.with_constants(desc, constants), inp, B)
    try:
        for source in ("zero", "al"):
            restore(p, inp)
            plan = check_plan_gains(p, cfg, inp, systems, source, penalties(cfg), f"{case} T={T} {source} {constants}", stats, constants=constants)
            pen = penalties(cfg)[1]
            for i in (0, 1):
                at = oracle_gains(systems[i], inp["A"], inp["b"], plan["lam"][i], plan["U"][i], pen, constants=constants)
                assert gn.reg_moves_the_gains(at[:2], oracle_gains(systems[i], inp["A"], inp["b"], plan["lam"][i], plan["U"][i], pen)[:2]), \
                    f"{case} T={T} {source}: reg does not move the gains of instance {i}"
        lam, U = multipliers_and_controls(p, cfg, inp)
        check_bits(p, inp, lam, U, penalties(cfg)[1], f"{case} T={T} {constants} bits")
    finally:
        p.close()


# ----------------------------------------------------------------------------------------------------------- (b), (d)

def multipliers_and_controls(p, cfg, inp):
    """lam, U of the case's AL solve of NIT iterations: multipliers that are positive on some rows, controls that are no start's."""
    restore(p, inp)
    al = cfg["al"]
    p.solve_al(NIT, al["lag"], al["penalty"], al["scaling"], True, False)
    return p.lam(), p.U()


def check_bits(p, inp, lam, U, pen, tag):
    """(b) under the pins in force.  Returns (K, d) of gains_al."""
    A, b = inp["A"], inp["b"]
    p.set_constraints(A, b, lam)
    p.set_controls(U)
    p.solve_al(0, 2, pen, 1.0, True, False)
    p.gains_al(pen)
    Kg, dg, ag = p.K(), p.d(), p.alpha()
    p.set_constraints(A, b, lam)
    p.set_controls(U)
    p.solve_al(1, 2, pen, 1.0, True, False)
    Ks, ds, a, lam_after = p.K(), p.d(), p.alpha(), p.lam()
    restore(p, inp)
    assert np.all(ag == 1.0)
    fin = (p.status() & 1) == 0
    assert fin.any(), f"{tag}: no finite instance"
    assert np.all(np.isfinite(Kg[fin])) and np.all(np.isfinite(dg[fin])), f"{tag}: gains are not finite"
    assert np.array_equal(lam_after, np.asarray(lam, float)), f"{tag}: a one-iteration solve with lag 2 moved the multipliers"
    assert np.array_equal(Ks[fin], Kg[fin]), f"{tag}: K of gains_al() differs from a one-iteration solve's by {np.abs(Ks[fin] - Kg[fin]).max():.3e}"
    assert np.array_equal(ds[fin], a[fin, None, None] * dg[fin]), f"{tag}: d of a one-iteration solve is not alpha d of gains_al()"
    assert np.all(np.log2(a[fin]) == np.round(np.log2(a[fin]))), f"{tag}: alpha is no power of two"
    return Kg, dg


def _close(got, ref, tol):
    return bool(np.all(np.abs(got - ref) <= tol["atol"] + tol["rtol"] * np.abs(ref)))


def check_degenerate(p, cfg, inp, U, tag):
    """(d)"""
    A, b = inp["A"], np.asarray(inp["b"], float)
    al = cfg["al"]
    zero = np.zeros_like(inp["lambda0"])
    for what, bb, pen in (("far bounds", b + FAR, al["penalty"]), ("penalty 0", b, 0.0)):
        p.set_constraints(A, bb, zero)
        p.set_controls(U)
        p.solve_al(0, al["lag"], al["penalty"], al["scaling"], True, False)
        p.gains_al(pen)
        Ka, da = p.K(), p.d()
        p.gains()
        K0, d0 = p.K(), p.d()
        assert np.all(np.isfinite(K0)) and np.all(np.isfinite(Ka))
        assert _close(Ka, K0, K_TOL), f"{tag}, {what}: K of gains_al differs from gains() by {np.abs(Ka - K0).max():.3e}"
        assert _close(da, d0, D_TOL), f"{tag}, {what}: d of gains_al differs from gains() by {np.abs(da - d0).max():.3e}"
    restore(p, inp)


def check_rows_matter(p, cfg, inp, lam, U, pen, tag):
    """The case tests something: with these multipliers and bounds the AL gains are not the plain ones."""
    p.set_constraints(inp["A"], inp["b"], lam)
    p.set_controls(U)
    p.solve_al(0, 2, pen, 1.0, True, False)
    p.gains_al(pen)
    Ka, da = p.K(), p.d()
    p.gains()
    same = _close(Ka, p.K(), K_TOL) and _close(da, p.d(), D_TOL)
    restore(p, inp)
    assert not same, f"{tag}: the AL gains equal the plain gains: no row is active"


# ----------------------------------------------------------------------------------------------------------- (e)

def check_con_outputs(p, inp, case, tag, worst, S=3):
    """closed_loop_report_con on the gains p holds against the longdouble reference on the same rollout (tests/closed_loop_con.py (1)): con_max
    within its bound, con_steps and the counts exact at a con_tol halfway between two reference values; then closed_loop_cov_con (5)."""
    A, b = con.rows_of(inp, p.T)
    sw, sx = con.sigmas_of(case, p.dims.n_x, p.T)
    f = CON_SIGMA_SCALE.get((case, p.T), 1.0)
    sw, sx = f * sw, f * sx
    seed = con.SEED + S
    base = p.closed_loop_noise(S, seed, sw, sx, with_feedforward=False, want_X=True, want_U=True)
    assert np.all(np.isfinite(base.X)) and np.all(np.isfinite(base.U)), f"{tag}: non-finite execution"
    g, bound = con.reference(A, b, base.X, base.U)
    hi, arg, _ = con.ref_con_max(g)
    hi_bound = np.take_along_axis(bound.reshape(hi.shape + (-1,)), arg[..., None], axis=2)[..., 0]
    step_max, step_bound = g.max(axis=3), bound.max(axis=3)
    con_tol = con.halfway(hi.astype(np.float64), lambda t: not np.any(np.abs(step_max - t) <= step_bound))
    r = p.closed_loop_report_con(con_tol, samples=S, seed=seed, sigma_w=sw, sigma_x0=sx, with_feedforward=False)
    dev = np.abs(r.con_max.astype(np.longdouble) - hi)
    worst["con_max"] = max(worst["con_max"], float((dev / hi_bound).max()))
    assert np.all(dev <= hi_bound), f"{tag}: con_max is {float((dev / hi_bound).max()):.3g} bounds from the reference"
    assert np.array_equal(r.con_steps, (step_max > con_tol).sum(axis=2).astype(np.float64)), f"{tag}: con_steps differs from the reference"
    assert np.array_equal(r.con_stats[:, 4], (hi > con_tol).sum(axis=1).astype(np.float64)), f"{tag}: n_con differs from the reference"
    assert np.array_equal(r.cost, base.cost)
    con.check_cov(p, A, b, case, tag, False, worst)


def check_execution(ctx, p, cfg, desc, inp, systems, plan, case, tag, rep, cov, worst):
    """(e) on the plan whose AL gains p holds."""
    st = gn.check_execution(ctx, p, cfg, desc, systems, plan, tag, cov)
    for k in rep:
        rep[k] = max(rep[k], st[k]) if k.startswith("worst") else rep[k] + st[k]
    check_con_outputs(p, inp, case, tag, worst)


# ----------------------------------------------------------------------------------------------------------- (f), (g)

def check_final_penalty(fp):
    """(g): fp(nb_iter, lag, penalty, scaling) is the solver's own double, for iteration counts that are multiples of the lag and not."""
    for n, lag, pen, sc in ((0, 2, 0.25, 1.1), (1, 2, 0.25, 1.1), (6, 2, 0.25, 1.1), (7, 2, 0.25, 1.1), (20, 5, 0.25, 1.1), (8, 3, 0.3, 1.7), (5, 1, 1e-3, 10.0)):
        want = final_penalty(n, lag, pen, sc)
        assert fp(n, lag, pen, sc) == want, (n, lag, pen, sc)
        assert want == pp.al_penalty(dict(penalty=pen, scaling=sc), n // lag)


def check_penalty_of_last_update(p, cfg, inp, tag):
    """(g): the penalty final_penalty names is the one solve_al used: a solve of `lag` iterations updates the multipliers once, in its last iteration,
    to max(0, lam0 + pen (A [x; u] - b)) on the trajectory it leaves -- with pen = final_penalty(lag, ..), within the rounding of that expression."""
    al = cfg["al"]
    restore(p, inp)
    p.solve_al(al["lag"], al["lag"], al["penalty"], al["scaling"], True, False)
    X, U, lam, fin = p.X(), p.U(), p.lam(), (p.status() & 1) == 0
    pen = final_penalty(al["lag"], al["lag"], al["penalty"], al["scaling"])
    assert pen != al["penalty"]
    n = 0
    for i in np.flatnonzero(fin):
        v, bound = pp.multiplier_update(inp["lambda0"][i], X[i], U[i], inp["A"], inp["b"], pen)
        ref = np.maximum(v, 0)
        assert np.all(np.abs(lam[i] - ref) <= bound), f"{tag}: the multipliers of instance {i} are not those of an update with final_penalty"
        n += int(np.any(ref > 0))
    assert n, f"{tag}: no multiplier is positive after the update: the check sees no penalty"


def check_state_machine(ctx, batch_solvers, psi_of=None, case="C3-m1", T=9):
    """(f)"""
    cfg, desc, inp, _ = make_case(ctx, case, T)
    al = cfg["al"]
    pen = al["penalty"]
    refused = cl._refused
    q = workloads.load_batch(ctx, desc, {k: v for k, v in inp.items() if k not in ("A", "b", "lambda0")}, B)
    try:   # no constraint rows: refused before and after a solve, by a text that names the remedy
        refused(lambda: q.gains_al(pen), NO_ROWS)
        q.solve_recursive(1, True, False)
        refused(lambda: q.gains_al(pen), NO_ROWS)
        refused(lambda: q.gains_al(pen), "ilqr_problem_set_constraints")
        q.gains()   # the plain call stays what it was
    finally:
        q.close()
    p = workloads.load_batch(ctx, desc, inp, B)
    try:
        refused(lambda: p.gains_al(pen), NO_PLAN)                       # nothing solved yet
        refused(lambda: p.gains_al(pen), "ilqr_solve_al with nb_iter = 0 rolls out the controls as they are")
        p.solve_al(0, al["lag"], pen, al["scaling"], True, False)
        refused(lambda: p.closed_loop(samples=1), "closed loop needs the gains")
        for bad in (float("nan"), -1.0, float("inf"), -0.25):
            refused(lambda: p.gains_al(bad), BAD_PENALTY)
        refused(lambda: p.closed_loop(samples=1), "closed loop needs the gains")   # a refused call leaves no gains
        p.gains_al(pen)                                                   # accepted after a 0-iteration solve
        p.closed_loop(samples=1)
        p.gains_al(0.0)                                                   # and with penalty 0
        setters = (lambda: p.set_init_state(inp["q0"], inp["dq0"]), lambda: p.set_keypoint_targets(0, inp["targets"][0]), lambda: p.set_controls(inp["U0"]),
                   lambda: p.set_constraints(inp["A"], inp["b"], inp["lambda0"]), lambda: p.reset_multipliers(), lambda: p.warm_start(0))
        for setter in setters:
            p.solve_al(1, al["lag"], pen, al["scaling"], True, False)
            p.gains_al(pen)
            setter()
            refused(lambda: p.gains_al(pen), NO_PLAN)
            refused(lambda: p.closed_loop(samples=1), "closed loop needs the gains")
        p.solve_recursive(2, True, True)                                  # accepted after each solver
        p.gains_al(pen)
        p.solve_al(2, al["lag"], pen, al["scaling"], True, True)
        p.gains_al(pen)
        Ka = p.K()
        p.closed_loop_cov(1e-3)
        p.track(0, p.X()[:, 0], True)
        p.gains()                                                         # a later gains() overwrites the records with the plain gains
        K0 = p.K()
        p.gains_al(pen)
        assert np.array_equal(p.K(), Ka) and not np.array_equal(K0, Ka)
        p.solve_al(0, al["lag"], pen, al["scaling"], True, False)         # a solve invalidates the gains (a 0-iteration one leaves none)
        refused(lambda: p.closed_loop(samples=1), "closed loop needs the gains")
        if batch_solvers:
            psi = psi_of(dict(kind="unitstep", K=2), cfg["T"], p.dims.n_u)
            for solve in (lambda: p.solve_batch_cp(psi, 2, True), lambda: p.solve_batch(2, True)):
                solve()
                refused(lambda: p.closed_loop(samples=1), "closed loop needs the gains")
                p.gains_al(pen)
                p.closed_loop(samples=1)
        ctx.synchronize()
    finally:
        p.close()
