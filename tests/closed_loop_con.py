"""Closed-loop executions and their covariance judged against the AL constraint rows (ilqr_problem_closed_loop_report_con,
ilqr_problem_closed_loop_cov_con) -- the reference and the checks shared by tests/tools/hostsim/closed_loop_con_checks.py (host build of the
generic kernels) and tests/test_gpu_closed_loop_con.py (device kernels).  The constraint sets are those of tests/al_shapes.make_case; every
case runs on the gains of a 3-iteration solve_al and on those of gains() afterwards.

  (1) reference: closed_loop_noise with the same seed returns X and U of the same rollout (same bits); NumPy gives g = A [x; u] - b in
      np.longdouble.  con_max agrees within 1e-12 (sum_j |A_j| |xu_j| + |b|) at the arg-max; con_steps and the counts are exact.  con_tol is
      halfway between two neighbouring reference values of con_max -- of all such pairs the one that lies between the samples of the most
      instances (halfway) -- and once equal to a reported con_max (strictness);
  (2) precondition, on the NumPy reference alone: for at least a quarter of the instances some sample has con_max > con_tol and some has not.
      One sample cannot lie on both sides, so at S = 1 the condition is asked of the batch: some instance above, some not.  Also on the
      reference alone: no step maximum lies within the bound of (1) of a halfway con_tol (the count would not be defined; such pairs are
      passed over).  WIDE_SPREAD lists the two (case, T) where the per-call form cannot hold, with the figures, and what is asserted there;
  (3) bit equalities: cost, stats and the four report outputs equal closed_loop_report's; cooperative = generic for the four new outputs
      (device only); a cut-out of batch and samples with its offsets reproduces the large call; closed_loop_noise and closed_loop_report
      called afterwards return their previous bytes;
  (4) reductions against NumPy with a planted NaN start state: counts and maxima exact, means 1e-12; outcome_con consistent with outcome;
  (5) covariance: con_var and con_z against NumPy built from closed_loop_cov(want_Sigma=True), K() and A, 1e-9 relative plus 1e-30 (con_z:
      plus the rounding of its own margin, numpy_con_cov -- the bounds sit on the middle instance's plan, whose margin is rounding alone); +inf with
      all sigmas 0; negative on a plan made to violate a row; the row kernel against the generic one to 1e-9 (device); the outputs of `out`
      array_equal to closed_loop_cov's;
  (6) sampled against analytic: C3, B = 2, T = 9, S = 4096, sigma_w = 1e-3: the sample variance of g[k][r] within 5 sqrt(2 / S) relative of
      con_var at every (k, r) (fixed seed);
  (7) interfaces: every refusal by its text, device pointers, reductions only.

Sigmas and seeds (SCALES, SEED) were picked on the host build so that (2) holds in every case, horizon and sample count the drivers run (but for
WIDE_SPREAD), and hold on the device's rollouts as well."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ilqr_planner_amd import capi, workloads
from tests import al_shapes as als
from tests import closed_loop as cl
from tests import closed_loop_noise as cn
from tests import closed_loop_report as cr
from tests import gains as gn

B = 13
NIT = 3
HORIZONS = (2, 3, 9, 10)
SEED = 90210
# case -> (workload, m, layout, per_step)
CASES = {
    "C3-m1": ("C3", 1, "state", False),
    "C3-m4": ("C3", 4, "state", False),
    "C3-m5-dense": ("C3", 5, "dense", False),
    "C2ndal-m2-control": ("C2ndal", 2, "control", False),
    "C4t1al-m2-control-per_step": ("C4t1al", 2, "control", True),
    "C4al-m16": ("C4al", 16, "state", False),
    "chain3-m1": ("chain3", 1, "state", False),
}
# (sigma_w scale, sigma_x0 scale) of cn.sigma_vectors per case: large enough that the samples of one instance lie on both sides of the batch's
# middle con_max (2), small enough that every execution stays finite
SCALES = {
    "C3-m1": (1e-1, 3e-1), "C3-m4": (2e-1, 3e-1), "C3-m5-dense": (1e-1, 3e-1), "C2ndal-m2-control": (3e-2, 3e-1),
    "C4t1al-m2-control-per_step": (3e-3, 3e-1), "C4al-m16": (1e-3, 3e-2), "chain3-m1": (3e-2, 3e-1),
}
SCALES_AT = {("C4al-m16", 2): (1e-3, 1e-1), ("C4al-m16", 3): (1e-3, 1e-1)}   # (case, T) -> scales: short horizons bear a larger start perturbation
# (case, T) where (2) cannot hold per call.  The 16 rows of C4al bound every state by the batch median of its maximum, so con_max -- the worst
# row -- spreads over 0.6 .. 5 between the instances, while the executions of PosOrnTime-2 stay finite only for start perturbations of a few
# 1e-2 (measured on the host build: with 0.3 on the joint positions alone the plans of three AL iterations run to 1e300 at T = 9 and 10; with
# 3e-2 an instance's samples spread by 0.02 .. 0.1, and 1 to 3 instances share a con_tol).  There the call is held to the batch form of (2),
# some instance above con_tol and some not, and the case as a whole to (2) through its calls at T = 2 and 3 (12 or 13 instances of 13).
WIDE_SPREAD = (("C4al-m16", 9), ("C4al-m16", 10))
CON_FIELDS = ("con_max", "con_steps", "con_stats", "outcome_con")
REP_FIELDS = ("cost", "stats", "kp_err", "kp_stats", "lim_cost", "outcome")


# ----------------------------------------------------------------------------------------------------------- cases

def make_case(ctx, case, T, bs=None):
    """(cfg, desc, inp) of a case; bs: a slice of the batch (the rows are those of the whole batch)."""
    name, m, layout, per_step = CASES[case]
    if name == "chain3":   # one row on joint 1 of the 3-joint chain: its bound is the batch median of the unconstrained plan's maximum
        cfg, desc, inp, _ = cl.make_case(ctx, "chain3", T)
        p = workloads.load_batch(ctx, desc, inp, B)
        try:
            p.solve_recursive(NIT, True, True)
            X = p.X()
        finally:
            p.close()
        A = np.zeros((1, 6))
        A[0, 1] = 1.0
        cfg = dict(cfg, solver="al", al=dict(gn.AL))
        inp = dict(inp, A=A, b=np.array([np.median(X[:, : T - 1, 1].max(axis=1))]), lambda0=np.zeros((B, T - 1, 1)))
    else:
        cfg, desc, inp = als.make_case(ctx, name, T, m, layout, per_step, nb_iter=NIT)
    if bs is not None:
        inp = cn.cut_inputs(inp, bs)
    return cfg, desc, inp


def solve(ctx, cfg, desc, inp):
    p = workloads.load_batch(ctx, desc, inp, len(inp["q0"]))
    workloads.run_solver(p, cfg, nb_iter=NIT, early_stop=True)
    return p


def rows_of(inp, T):
    """(A [T-1][m][n], b [T-1][m]) of a case's inputs"""
    A, b = np.asarray(inp["A"], float), np.asarray(inp["b"], float)
    if A.ndim == 2:
        A, b = np.broadcast_to(A, (T - 1,) + A.shape), np.broadcast_to(b, (T - 1,) + b.shape)
    return A, b


def sigmas_of(case, nx, T=9):
    """cn.sigma_vectors (graded, with entries that are not drawn), but every start entry drawn: at T = 2 the one judged step is k = 0, and a
    state row sees only the start perturbation there"""
    scale_w, scale_x0 = SCALES_AT.get((case, T), SCALES[case])
    sw, _ = cn.sigma_vectors(nx, scale_w, scale_x0)
    return sw, scale_x0 * (1.0 - 0.046875 * np.arange(nx))


# ----------------------------------------------------------------------------------------------------------- reference

def reference(A, b, X, U):
    """g [B][S][T-1][m] in longdouble and the bound of (1) for every g: 1e-12 (sum_j |A_j| |xu_j| + |b|)"""
    Z = np.concatenate([X[:, :, :-1, :], U], axis=3).astype(np.longdouble)
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    with np.errstate(invalid="ignore"):
        g = np.einsum("krj,bskj->bskr", Al, Z) - bl[None, None]
        bound = 1e-12 * (np.einsum("krj,bskj->bskr", np.abs(Al), np.abs(Z)) + np.abs(bl)[None, None])
    return g, bound


def ref_con_max(g):
    """con_max [B][S] of the reference (NaN where a g is not finite) and the index of its arg-max"""
    Bn, S = g.shape[:2]
    flat = g.reshape(Bn, S, -1)
    bad = ~np.all(np.isfinite(flat), axis=2)
    arg = np.argmax(np.where(np.isfinite(flat), flat, -np.inf), axis=2)
    hi = np.take_along_axis(flat, arg[..., None], axis=2)[..., 0]
    return np.where(bad, np.nan, hi), arg, bad


def straddled(hi, con_tol):
    """How many instances have a finite sample above con_tol and one that is not (S = 1: whether the batch has both)"""
    with np.errstate(invalid="ignore"):
        above = hi > con_tol
    fin = np.isfinite(hi)
    if hi.shape[1] == 1:
        return int(np.any(above & fin) and np.any(~above & fin))
    return int(np.count_nonzero(np.any(above & fin, axis=1) & np.any(~above & fin, axis=1)))


def halfway(hi, usable=None):
    """con_tol of a call: halfway between two neighbouring distinct values of con_max [B][S] (finite ones) -- of all such, the one that lies
    between the samples of the most instances (the first of them; S = 1: the one nearest the middle).  usable(t): a condition on the
    candidates (check_sampled_call: no step maximum of the reference within its bound of t -- where the feedback has pulled two executions
    onto the plan, two values of con_max can lie 1e-13 apart, and a count against a threshold between them is not defined)."""
    v = np.unique(np.asarray(hi, dtype=np.float64)[np.isfinite(hi)])
    assert len(v) >= 2, "con_max takes one value only: the case tests nothing"
    mid = [float(t) for t in 0.5 * (v[:-1] + v[1:]) if usable is None or usable(float(t))]
    assert mid, "no value halfway between two neighbouring con_max is usable"
    if hi.shape[1] == 1:
        return min(mid, key=lambda t: abs(np.count_nonzero(v > t) - len(v) / 2))
    return mid[int(np.argmax([straddled(hi, t) for t in mid]))]


def precondition(hi, con_tol, tag, per_call=True):
    """(2) on the reference's con_max [B][S]"""
    n = straddled(hi, con_tol)
    if hi.shape[1] == 1 or not per_call:
        with np.errstate(invalid="ignore"):
            n = int(np.any(hi > con_tol) and np.any(hi <= con_tol))
        assert n, f"{tag}: every instance lies on one side of con_tol: the case tests nothing"
    else:
        assert 4 * n >= hi.shape[0], f"{tag}: only {n} of {hi.shape[0]} instances have samples on both sides of con_tol: the case tests nothing"


def numpy_con_stats(con_max, con_steps, con_tol):
    Bn, S = con_max.shape
    out = np.empty((Bn, 6))
    for b_ in range(Bn):
        good = np.isfinite(con_max[b_])
        v, q = con_max[b_][good], con_steps[b_][good]
        n = len(v)
        out[b_] = [v.astype(np.longdouble).sum() / n if n else np.nan, v.max() if n else np.nan, q.astype(np.longdouble).sum() / n if n else np.nan,
                   q.max() if n else np.nan, np.count_nonzero(v > con_tol), S - n]
    return out


def numpy_outcome_con(r, kp_tol, lim_tol, con_tol):
    kp_tol = np.broadcast_to(np.asarray(kp_tol, dtype=np.float64), r.kp_err.shape[2:])
    _, miss, lim = cr.numpy_outcome(r.cost, r.kp_err, r.lim_cost, kp_tol, lim_tol)
    bad = ~np.isfinite(r.cost)
    with np.errstate(invalid="ignore"):
        con = ((r.con_max > con_tol) | ~np.isfinite(r.con_max)) & ~bad
    ok = ~bad & ~miss & ~lim & ~con
    return np.stack([ok.sum(1), miss.sum(1), lim.sum(1), con.sum(1), bad.sum(1)], axis=1).astype(np.float64)


def check_reductions(r, kp_tol, lim_tol, con_tol, tag):
    """(4) of a call with every output, against NumPy on its own per-sample arrays"""
    ref = numpy_con_stats(r.con_max, r.con_steps, con_tol)
    S = r.con_max.shape[1]
    assert np.array_equal(r.con_stats[:, [1, 3, 4, 5]], ref[:, [1, 3, 4, 5]], equal_nan=True), f"{tag}: maxima / counts of con_stats {r.con_stats.tolist()} != {ref.tolist()}"
    some = ref[:, 5] < S
    assert np.all(np.isnan(r.con_stats[~some][:, :4])), f"{tag}: no good sample must give NaN"
    np.testing.assert_allclose(r.con_stats[some][:, [0, 2]], ref[some][:, [0, 2]], rtol=1e-12, atol=0, err_msg=f"{tag}: means of con_stats")
    if r.outcome_con is not None:
        out = numpy_outcome_con(r, kp_tol, lim_tol, con_tol)
        assert np.array_equal(r.outcome_con, out), f"{tag}: outcome_con {r.outcome_con.tolist()} != {out.tolist()}"
        assert np.array_equal(r.outcome_con[:, [1, 2, 4]], r.outcome[:, [1, 2, 3]]), f"{tag}: n_miss, n_lim, n_bad of outcome_con are not those of outcome"
        assert np.all(r.outcome_con[:, 0] <= r.outcome[:, 0]), f"{tag}: n_ok of outcome_con exceeds that of outcome"


def _same(a, b_, what, tag):
    for f in what:
        x, y = getattr(a, f), getattr(b_, f)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y, equal_nan=True)), f"{tag}: {f} differs"


# ----------------------------------------------------------------------------------------------------------- sampled

def check_sampled_call(p, A, b, case, S, seed, tag, compare_generic, worst, with_ff=True, per_call=True):
    """(1)-(4) of one plan at one sample count; the feed-forward term is on at odd S where with_ff allows it"""
    nx = p.dims.n_x
    sw, sx = sigmas_of(case, nx, p.T)
    ff = bool(S % 2) and with_ff
    base = p.closed_loop_noise(S, seed, sw, sx, with_feedforward=ff, want_X=True, want_U=True)
    assert np.all(np.isfinite(base.X)) and np.all(np.isfinite(base.U)), f"{tag}: non-finite execution"
    g, bound = reference(A, b, base.X, base.U)
    hi, arg, _ = ref_con_max(g)
    hi_bound = np.take_along_axis(bound.reshape(hi.shape + (-1,)), arg[..., None], axis=2)[..., 0]
    step_max = g.max(axis=3)
    step_bound = bound.max(axis=3)
    con_tol = halfway(hi.astype(np.float64), lambda t: not np.any(np.abs(step_max - t) <= step_bound))
    precondition(hi, con_tol, tag, per_call)
    worst["straddled"] = min(worst.get("straddled", B), straddled(hi, con_tol)) if S > 1 and per_call else worst.get("straddled", B)
    assert not np.any(np.abs(step_max - con_tol) <= step_bound), f"{tag}: a step maximum of the reference lies within the bound of con_tol"
    kw = dict(samples=S, seed=seed, sigma_w=sw, sigma_x0=sx, with_feedforward=ff)
    plain = p.closed_loop_report(**kw)
    tol = cr.median_tolerances(plain.kp_err)
    rep = p.closed_loop_report(**kw, kp_tol=tol, lim_tol=0.0)
    r = p.closed_loop_report_con(con_tol, **kw, kp_tol=tol, lim_tol=0.0)
    # (1)
    dev = np.abs(r.con_max.astype(np.longdouble) - hi)
    ratio = float((dev / hi_bound).max())
    worst["con_max"] = max(worst["con_max"], ratio)
    print(f"{tag}: con_max worst {ratio:.3e} of its bound (|dev| {float(dev.max()):.3e}), con_tol {con_tol:.6g}, "
          f"{np.count_nonzero(hi > con_tol)} of {hi.size} above", flush=True)
    assert np.all(dev <= hi_bound), f"{tag}: con_max is {ratio:.3g} bounds from the reference"
    ref_steps = (step_max > con_tol).sum(axis=2).astype(np.float64)
    assert np.array_equal(r.con_steps, ref_steps), f"{tag}: con_steps differs from the reference at {np.argwhere(r.con_steps != ref_steps)[:3].tolist()}"
    assert np.array_equal(r.con_stats[:, 4], (hi > con_tol).sum(axis=1).astype(np.float64)), f"{tag}: n_con differs from the reference"
    assert not r.con_stats[:, 5].any()
    # (3)
    _same(r, rep, REP_FIELDS, f"{tag}: closed_loop_report")
    assert np.array_equal(r.cost, base.cost) and np.array_equal(r.stats, base.stats), f"{tag}: closed_loop_noise"
    # (4)
    check_reductions(r, tol, 0.0, con_tol, tag)
    # strictness: con_tol equal to a reported con_max
    eq = float(np.sort(r.con_max.ravel())[r.con_max.size // 2])
    e = p.closed_loop_report_con(eq, **kw, kp_tol=tol, lim_tol=0.0)
    assert np.array_equal(e.con_max, r.con_max), f"{tag}: con_max moves with con_tol"
    assert np.array_equal(e.con_stats[:, 4], (r.con_max > eq).sum(axis=1).astype(np.float64)), f"{tag}: a con_tol equal to a con_max"
    assert np.all(e.con_steps[r.con_max == eq] == 0) and np.all(e.con_steps[r.con_max > eq] >= 1) and np.all(e.con_steps[r.con_max < eq] == 0), f"{tag}: con_steps at a con_tol equal to a con_max"
    lo, hi_n = (step_max > eq + step_bound).sum(axis=2), (step_max > eq - step_bound).sum(axis=2)
    assert np.all((lo <= e.con_steps) & (e.con_steps <= hi_n)), f"{tag}: con_steps at a con_tol equal to a con_max, against the reference"
    check_reductions(e, tol, 0.0, eq, tag + " equal")
    # without tolerances: no outcome_con; without `out`
    n = p.closed_loop_report_con(con_tol, **kw, want_kp_err=False, want_lim_cost=False)
    assert n.outcome_con is None and n.kp_err is None and n.outcome is None
    _same(n, r, ("cost", "stats", "con_max", "con_steps", "con_stats"), f"{tag}: the call without `out`")
    if compare_generic:
        with cl.generic_pin():
            gk = p.closed_loop_report_con(con_tol, **kw, kp_tol=tol, lim_tol=0.0)
        _same(r, gk, REP_FIELDS + CON_FIELDS, f"{tag}: the generic kernel")
    # the calls that existed before still return their bytes
    after = p.closed_loop_noise(S, seed, sw, sx, with_feedforward=ff, want_X=True, want_U=True)
    _same(after, base, ("cost", "stats", "X", "U"), f"{tag}: closed_loop_noise afterwards")
    _same(p.closed_loop_report(**kw, kp_tol=tol, lim_tol=0.0), rep, REP_FIELDS, f"{tag}: closed_loop_report afterwards")
    return con_tol, tol


def check_planted_nan(p, case, tag):
    """(4): one NaN start state is bad everywhere and leaves every other number untouched"""
    S = 5
    X0 = p.X()[:, 0, :]
    sw, sx = sigmas_of(case, p.dims.n_x, p.T)
    centre = np.repeat(X0[:, None, :], S, axis=1)
    kw = dict(samples=S, seed=SEED, sigma_w=sw, sigma_x0=sx)
    first = p.closed_loop_report_con(0.0, x0=centre, **kw)
    con_tol = float(halfway(first.con_max))
    tol = cr.median_tolerances(first.kp_err)
    clean = p.closed_loop_report_con(con_tol, x0=centre, kp_tol=tol, lim_tol=0.0, **kw)
    centre[3, 1, 0] = np.nan
    r = p.closed_loop_report_con(con_tol, x0=centre, kp_tol=tol, lim_tol=0.0, **kw)
    keep = np.ones((p.B, S), dtype=bool)
    keep[3, 1] = False
    assert np.isnan(r.con_max[3, 1]) and np.isnan(r.cost[3, 1]) and r.con_steps[3, 1] == 0, f"{tag}: the planted sample is not bad"
    assert np.array_equal(r.con_max[keep], clean.con_max[keep]) and np.array_equal(r.con_steps[keep], clean.con_steps[keep])
    check_reductions(r, tol, 0.0, con_tol, tag)
    rest = np.arange(p.B) != 3
    assert np.array_equal(r.con_stats[rest], clean.con_stats[rest]) and np.array_equal(r.outcome_con[rest], clean.outcome_con[rest]), f"{tag}: another instance moved"
    assert r.con_stats[3, 5] == 1 and r.outcome_con[3, 4] == 1, f"{tag}: the bad sample is not counted once"


def check_case(ctx, case, T, samples, compare_generic=False, worst=None, cov=True):
    """One case at one horizon: both sets of gains, every S of `samples`; the planted NaN; the covariance checks (5)."""
    worst = worst if worst is not None else dict(con_max=0.0, con_var=0.0)
    cfg, desc, inp = make_case(ctx, case, T)
    A, b = rows_of(inp, T)
    p = solve(ctx, cfg, desc, inp)
    try:
        for source in ("al", "gains"):
            if source == "gains":
                p.gains()
            for S in samples:
                # the feed-forward of gains() is the whole Newton step of a plan of three iterations: on the time systems a loop that adds it at
                # every step leaves every bound (tests/gains.check_execution), so there it stays off
                check_sampled_call(p, A, b, case, S, SEED + S, f"{case} T={T} {source} S={S}", compare_generic, worst,
                                   with_ff=not (source == "gains" and cfg.get("ctimes")), per_call=(case, T) not in WIDE_SPREAD)
            if cov:
                check_cov(p, A, b, case, f"{case} T={T} {source}", compare_generic, worst)
        if T == 9:
            check_planted_nan(p, case, f"{case} T={T} planted")
    finally:
        p.close()
    return f"{case} T={T} S={tuple(samples)}: con_max at most {worst['con_max']:.3e} of its bound, con_var at most {worst['con_var']:.3e} relative so far"


def check_cut_out(ctx, case):
    """(3): instances 2 .. 10 and samples 1 .. 13 of a 13 x 17 call as a call of their own"""
    T, S = 9, 17
    cfg, desc, inp = make_case(ctx, case, T)
    p = solve(ctx, cfg, desc, inp)
    try:
        sw, sx = sigmas_of(case, p.dims.n_x, p.T)
        first = p.closed_loop_report_con(0.0, samples=S, seed=SEED, sigma_w=sw, sigma_x0=sx, with_feedforward=True)
        con_tol = float(halfway(first.con_max))
        big = p.closed_loop_report_con(con_tol, samples=S, seed=SEED, sigma_w=sw, sigma_x0=sx, with_feedforward=True)
    finally:
        p.close()
    bs, ss_ = slice(2, 11), slice(1, 14)
    q = solve(ctx, cfg, desc, cn.cut_inputs(inp, bs))
    try:
        small = q.closed_loop_report_con(con_tol, samples=13, seed=SEED, sigma_w=sw, sigma_x0=sx, with_feedforward=True, instance_offset=2, sample_offset=1)
    finally:
        q.close()
    for f in ("cost", "kp_err", "lim_cost", "con_max", "con_steps"):
        assert np.array_equal(getattr(big, f)[bs, ss_], getattr(small, f)), f"{case}: {f} of the cut-out differs from the large call"
    assert np.any(big.con_steps[bs, ss_] > 0) and np.any(big.con_steps[bs, ss_] == 0), f"{case}: the cut-out lies on one side of con_tol"


# ----------------------------------------------------------------------------------------------------------- covariance

def numpy_con_cov(A, b, X, U, K, Sigma):
    """(con_var [B][T-1][m], con_z [B], slack [B]) in longdouble from Sigma [B][T][n][n] and K [B][T-1][n_u][n].  slack: the bounds are batch
    medians of the plans' own maxima, so the middle instance of a row sits ON its bound and its margin is rounding alone (1e-14 against 0.0
    measured); 1e-9 relative of such a con_z means nothing, and the margin's rounding, 1e-12 (sum_j |A_j| |xu_j| + |b|) / sqrt(con_var), is
    allowed on top of it."""
    nx = X.shape[2]
    Al = A.astype(np.longdouble)
    c = Al[None, :, :, :nx] + np.einsum("kri,bkij->bkrj", Al[:, :, nx:], K.astype(np.longdouble))   # [B][T-1][m][n]
    var = np.einsum("bkri,bkij,bkrj->bkr", c, Sigma[:, :-1].astype(np.longdouble), c)
    Z = np.concatenate([X[:, :-1], U], axis=2).astype(np.longdouble)
    margin = b.astype(np.longdouble)[None] - np.einsum("krj,bkj->bkr", Al, Z)
    mag = np.abs(b.astype(np.longdouble))[None] + np.einsum("krj,bkj->bkr", np.abs(Al), np.abs(Z))
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.sqrt(np.where(var > 0, var, 1))
        z = np.where(var > 0, margin / sd, np.inf).reshape(len(X), -1)
    arg = z.argmin(axis=1)[:, None]
    # what the margin's own rounding moves z by, at the arg-min: b - A [xbar; ubar] is a difference of numbers of size mag (the form of (1)'s bound)
    slack = np.take_along_axis((1e-12 * mag / sd).reshape(len(X), -1), arg, axis=1)[:, 0]
    return var, np.take_along_axis(z, arg, axis=1)[:, 0], np.where(np.isfinite(z.min(axis=1)), slack, 0.0)


def _close_z(got, ref, slack):
    """1e-9 relative plus 1e-30, plus the margin's rounding (numpy_con_cov); +inf (no row with a positive variance) must be +inf on both sides"""
    with np.errstate(invalid="ignore"):
        return bool(np.all((got == ref) | (np.abs(got - ref) <= 1e-9 * np.abs(ref) + 1e-30 + slack)))


def check_cov(p, A, b, case, tag, compare_generic, worst):
    """(5) on the plan and gains p holds"""
    nx = p.dims.n_x
    sw, sx = cn.sigma_vectors(nx, 1e-3, 1e-2)
    X, U, K = p.X(), p.U(), p.K()
    full = p.closed_loop_cov(sw, sx, want_Sigma=True)
    r = p.closed_loop_cov_con(sw, sx, want_Sigma=True, want_kp_Sigma=True, want_kp_var=True, want_u_var=True, want_lim_z=True)
    _same(r, full, ("Sigma", "kp_Sigma", "kp_var", "u_var", "lim_z"), f"{tag}: the outputs of closed_loop_cov")
    var, z, slack = numpy_con_cov(A, b, X, U, K, full.Sigma)
    dev = np.abs(r.con_var - var)
    rel = float((dev / (np.abs(var) + 1e-30 / 1e-9)).max())
    worst["con_var"] = max(worst["con_var"], rel)
    assert np.all(dev <= 1e-9 * np.abs(var) + 1e-30), f"{tag}: con_var is {rel:.3e} relative from NumPy"
    assert np.all(r.con_var >= -1e-30)
    # con_z: the minimum over the (k, r) both sides call positive, within 1e-9 of the reference's
    assert _close_z(r.con_z, z, slack), f"{tag}: con_z {r.con_z.tolist()} against {z.astype(float).tolist()}"
    only = p.closed_loop_cov_con(sw, sx)
    assert only.Sigma is None and only.lim_z is None
    _same(only, r, ("con_var", "con_z"), f"{tag}: the call without `out`")
    for keep in (("con_var",), ("con_z",)):
        part = p.closed_loop_cov_con(sw, sx, want_con_var="con_var" in keep, want_con_z="con_z" in keep, want_lim_z=True)
        _same(part, r, keep + ("lim_z",), f"{tag}: the call for {keep}")
    zero = p.closed_loop_cov_con(None, None)
    assert not np.any(zero.con_var) and np.all(zero.con_z == np.inf), f"{tag}: zero sigmas give con_z {zero.con_z}"
    if compare_generic:
        with cl.generic_pin():
            gk = p.closed_loop_cov_con(sw, sx)
        assert np.all(np.abs(gk.con_var - r.con_var) <= 1e-9 * np.abs(r.con_var) + 1e-30), f"{tag}: con_var of the row kernel against the generic one"
        assert _close_z(gk.con_z, r.con_z, 2 * slack), f"{tag}: con_z of the row kernel against the generic one"
    _same(p.closed_loop_cov(sw, sx, want_Sigma=True), full, ("Sigma", "kp_Sigma", "kp_var", "u_var", "lim_z"), f"{tag}: closed_loop_cov afterwards")


def check_violated_plan(ctx, case="C3-m4", T=9):
    """(5): a plan made to violate a row (its bounds moved below the plan) has a negative con_z"""
    cfg, desc, inp = make_case(ctx, case, T)
    A, b = rows_of(inp, T)
    p = workloads.load_batch(ctx, desc, inp, B)
    try:
        p.solve_recursive(NIT, True, True)   # the unconstrained solver does not look at the rows: its plan is what they are moved below
        Z = np.concatenate([p.X()[:, :-1], p.U()], axis=2)
        low = (np.einsum("krj,bkj->bkr", A, Z)).min() - 0.5     # every row of every instance is violated by at least 0.5
        p.set_constraints(np.asarray(inp["A"]), np.full_like(np.asarray(inp["b"]), low), inp["lambda0"])   # (drops the plan and its gains)
        p.set_controls(inp["U0"])
        p.solve_recursive(NIT, True, True)   # the same solve again
        assert np.array_equal(np.concatenate([p.X()[:, :-1], p.U()], axis=2), Z)
        r = p.closed_loop_cov_con(1e-3, 1e-2)
        assert np.all(r.con_z < 0) and np.all(np.isfinite(r.con_z)), f"{case}: con_z of a violated plan {r.con_z.tolist()}"
        s = p.closed_loop_report_con(0.0, samples=4, seed=1, sigma_w=1e-5)
        assert np.all(s.con_max > 0.4) and np.all(s.con_stats[:, 4] == 4) and np.all(s.con_steps >= 1), f"{case}: a violated plan is feasible"
    finally:
        p.close()


def check_sampled_against_analytic(ctx, S=4096, T=9, Bn=2, seed=2024):
    """(6).  Returns the largest |sample variance / con_var - 1| in units of 5 sqrt(2 / S)."""
    case = "C3-m4"
    cfg, desc, inp = make_case(ctx, case, T, bs=slice(0, Bn))
    A, b = rows_of(inp, T)
    p = solve(ctx, cfg, desc, inp)
    try:
        sg = np.full(p.dims.n_x, 1e-3)
        base = p.closed_loop_noise(S, seed, sg, None, want_stats=False, want_X=True, want_U=True)
        cv = p.closed_loop_cov_con(sg, None)
    finally:
        p.close()
    g, _ = reference(A, b, base.X, base.U)
    sv = g.astype(np.float64).var(axis=1, ddof=1)   # [B][T-1][m]
    live = cv.con_var > 0   # k = 0 without a start perturbation: x_0 is the plan's, and the variance is 0 on both sides
    assert np.array_equal(live, np.broadcast_to((np.arange(T - 1) > 0)[None, :, None], live.shape)), "con_var must be positive from k = 1 on, and 0 at k = 0"
    assert np.all(sv[~live] <= 1e-24)
    rel = np.abs(sv[live] / cv.con_var[live] - 1.0)
    lim = 5.0 * np.sqrt(2.0 / S)
    assert np.all(rel <= lim), f"sample variance of g is {rel.max():.3e} relative from con_var (allowed {lim:.3e})"
    return float(rel.max() / lim)


# ----------------------------------------------------------------------------------------------------------- interfaces

def check_interfaces(ctx, device_call, device_cov_call):
    """(7).  device_call(p, S, nz, x0, ff, tol, con_tol, which) -> ClosedLoopReportCon through the _dev entry point (which: names of the
    outputs asked for); device_cov_call(p, sw, sx, which) -> ClosedLoopCovCon."""
    refused = cl._refused
    case, T = "C3-m4", 9
    cfg, desc, inp = make_case(ctx, case, T)
    plain_inp = {k: v for k, v in inp.items() if k not in ("A", "b", "lambda0")}
    p = workloads.load_batch(ctx, desc, plain_inp, B)
    try:
        refused(lambda: p.closed_loop_report_con(0.0, samples=2), "closed loop needs the gains")
        p.solve_recursive(NIT, True, True)
        refused(lambda: p.closed_loop_report_con(0.0, samples=2), "closed loop report con: no constraints set")
        refused(lambda: p.closed_loop_cov_con(1e-3), "closed loop cov con: no constraints set")
    finally:
        p.close()
    p = solve(ctx, cfg, desc, inp)
    try:
        refused(lambda: p.closed_loop_report_con(0.0, samples=0), "n_samples must be >= 1")
        refused(lambda: p.closed_loop_report_con(0.0, samples=2, seed=1, sigma_w=-1.0), "sigma_w and sigma_x0 must be finite and >= 0")
        refused(lambda: p.closed_loop_report_con(0.0, samples=2, lim_tol=np.nan), "a tolerance is NaN")
        refused(lambda: p.closed_loop_report_con(0.0, samples=2, lim_tol=-1.0), "lim_tol must be >= 0")
        refused(lambda: p.closed_loop_report_con(np.nan, samples=2), "closed loop report con: con_tol is NaN")
        buf = np.zeros(B * 2 * 8)
        co = capi.Con(outcome_con=buf.ctypes.data)
        refused(lambda: ctx.check(p.L.ilqr_problem_closed_loop_report_con(p.h, 2, None, None, None, 0, None, None, None, None, 0.0, C.byref(co))),
                "tol is a null pointer while outcome_con is asked for")
        rp = capi.Report(outcome=buf.ctypes.data)
        refused(lambda: ctx.check(p.L.ilqr_problem_closed_loop_report_con(p.h, 2, None, None, None, 0, None, None, None, C.byref(rp), 0.0, None)),
                "tol is a null pointer while kp_stats or outcome is asked for")
        none = capi.Con()
        for rp_, co_ in ((None, None), (None, C.byref(none)), (C.byref(capi.Report()), C.byref(none))):
            refused(lambda: ctx.check(p.L.ilqr_problem_closed_loop_report_con(p.h, 2, None, None, None, 0, None, None, None, rp_, 0.0, co_)),
                    "closed loop report con: con and out both ask for nothing")
        big = (1 << 31) // (B * p.dims.n_x) + 1
        co = capi.Con(con_max=buf.ctypes.data)
        refused(lambda: ctx.check(p.L.ilqr_problem_closed_loop_report_con(p.h, big, None, None, None, 0, None, None, None, None, 0.0, C.byref(co))),
                "B * n_samples * n_x overflows the kernels' 32-bit offsets")
        refused(lambda: p.closed_loop_cov_con(-1e-3), "sigma_w and sigma_x0 must be finite and >= 0")
        for cv_, co_ in ((None, None), (None, C.byref(capi.CovCon())), (C.byref(capi.Cov()), C.byref(capi.CovCon()))):
            refused(lambda: ctx.check(p.L.ilqr_problem_closed_loop_cov_con(p.h, None, None, cv_, co_)), "closed loop cov con: con and out both ask for nothing")
        # the report call still refuses a null `out`
        refused(lambda: ctx.check(p.L.ilqr_problem_closed_loop_report(p.h, 2, None, None, None, 0, None, None, None, None)), "every report output is a null pointer")
        refused(lambda: ctx.check(p.L.ilqr_problem_closed_loop_cov(p.h, None, None, None)), "every output is a null pointer")
        # device pointers; reductions only
        nx = p.dims.n_x
        sw, sx = sigmas_of(case, nx, p.T)
        x0 = p.X()[:, None, 0, :] + 0.01 * np.arange(5)[None, :, None]
        first = p.closed_loop_report_con(0.0, samples=5, seed=9, sigma_w=sw, sigma_x0=sx, x0=x0)
        con_tol = float(halfway(first.con_max))
        every = REP_FIELDS + CON_FIELDS
        host = p.closed_loop_report_con(con_tol, samples=5, seed=9, sigma_w=sw, sigma_x0=sx, x0=x0, with_feedforward=True, kp_tol=0.05, lim_tol=0.0)
        tol = p.tol(0.05, 0.0)
        dev = device_call(p, 5, p.noise(9, sw, sx), x0, True, tol, con_tol, every)
        _same(host, dev, every, "the device-pointer entry point")
        for which in (("con_stats", "outcome_con"), ("con_stats",), ("outcome_con",), ("con_steps",), ("con_max", "outcome")):
            only = device_call(p, 5, p.noise(9, sw, sx), x0, True, tol, con_tol, which)   # everything else in the problem's workspaces
            _same(host, only, which, f"{which} only, device pointers")
        only = p.closed_loop_report_con(con_tol, samples=5, seed=9, sigma_w=sw, sigma_x0=sx, x0=x0, with_feedforward=True, kp_tol=0.05, lim_tol=0.0,
                                        want_cost=False, want_stats=False, want_kp_err=False, want_lim_cost=False, want_kp_stats=False, want_outcome=False,
                                        want_con_max=False, want_con_steps=False)
        _same(host, only, ("con_stats", "outcome_con"), "reductions only")
        hostc = p.closed_loop_cov_con(1e-3, 1e-2, want_lim_z=True)
        for which in (("con_var", "con_z", "lim_z"), ("con_z",), ("con_var",)):
            devc = device_cov_call(p, 1e-3, 1e-2, which)
            _same(hostc, devc, which, f"{which}, covariance through device pointers")
        p.set_controls(inp["U0"])
        refused(lambda: p.closed_loop_report_con(0.0, samples=2), "closed loop needs the gains")
        refused(lambda: p.closed_loop_cov_con(1e-3), "closed loop needs the gains")
    finally:
        p.close()


SHAPES_DEV = dict(cost=lambda p, S: (p.B, S), stats=lambda p, S: (p.B, 5), kp_err=lambda p, S: (p.B, S, p.n_kp, 5), kp_stats=lambda p, S: (p.B, p.n_kp, 12),
                  lim_cost=lambda p, S: (p.B, S), outcome=lambda p, S: (p.B, 4), con_max=lambda p, S: (p.B, S), con_steps=lambda p, S: (p.B, S),
                  con_stats=lambda p, S: (p.B, 6), outcome_con=lambda p, S: (p.B, 5))
COV_FIELDS = ("Sigma", "kp_Sigma", "kp_var", "u_var", "lim_z", "con_var", "con_z")


def cov_shapes(p):
    nx, nk = p.dims.n_x, p.n_kp
    return dict(Sigma=(p.B, p.T, nx, nx), kp_Sigma=(p.B, nk, nx, nx), kp_var=(p.B, nk, 5), u_var=(p.B, p.T - 1, p.dims.n_u), lim_z=(p.B,),
                con_var=(p.B, p.T - 1, p.m), con_z=(p.B,))


def host_pointer_call(p, S, nz, x0, ff, tol, con_tol, which):
    """ilqr_problem_closed_loop_report_con_dev on arrays of the host: what a device pointer is on the host build of the kernels"""
    arr = {f: (np.zeros(SHAPES_DEV[f](p, S)) if f in which else None) for f in SHAPES_DEV}
    x0 = np.ascontiguousarray(x0) if x0 is not None else None
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    p.closed_loop_report_con_dev(S, nz, ptr(x0), None, ff, tol, con_tol, **{f + "_ptr": ptr(arr[f]) for f in SHAPES_DEV})
    p.ctx.synchronize()
    return capi.ClosedLoopReportCon(**arr)


def host_pointer_cov_call(p, sw, sx, which):
    sh = cov_shapes(p)
    arr = {f: (np.zeros(sh[f]) if f in which else None) for f in COV_FIELDS}
    p.closed_loop_cov_con_dev(sw, sx, **{f + "_ptr": (arr[f].ctypes.data if arr[f] is not None else None) for f in COV_FIELDS})
    p.ctx.synchronize()
    return capi.ClosedLoopCovCon(**arr)
