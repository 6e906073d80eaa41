"""Clearance under the closed-loop covariance (ilqr_problem_closed_loop_cov_clr) -- cases and checks shared by
tests/tools/hostsim/cov_clearance_checks.py (the host build) and tests/test_gpu_cov_clearance.py (the device kernels, under the generic pin and on
k_cl_cov_rows).  The problems, worlds and helpers are those of tests/clearance.py, tests/obstacles.py and tests/self_collision.py; the reference is
tests/cov_clearance_reference.py, which takes the library's own Sigma as data.

Shapes: T = 2, 3, 9; B = 1, 13, 70 (a partial wave, and two waves with a partial one); the Panda with a tool frame, gen7 and gen4 (four joints:
the index map and a 9 x 9 Sigma); PosOrn-1, PosOrn-2, PosOrnTime-2 and JointSpace-1 with a chain; 1, 5 and 32 spheres (link -1, a fixed segment
and the tool segment among them); 1 and 9 obstacles with an unused slot; 0 and 2 planes; 0, 1 and 7 self pairs on 1 and 3 anchors; traj_per_set
1, 5 and B.  Plans: 0-iteration rollouts of random controls with gains from ilqr_problem_gains, and 3-iteration solves.

(a) values      clr_var within 1e-12 S_abs, clr_z within the reference's per-entry bound, clr_z_min likewise; clr_z_at and eligible exactly; the
                _dev form on bytes; a subset of outputs on bytes.
(b) bit rules   sigmas times 2: clr_var times 4, clr_z halved, clr_z_at unchanged, bit for bit; `out` on the bytes of closed_loop_cov; closed_loop_cov
                and _cov_con unchanged by a call in between.
                Magnitudes: sigma is 1e-3 .. 1e-2, so Sigma's entries lie within 1e-10 .. 1e-1 and the form's products within 1e-20 .. 1: every
                intermediate is a normal double far from 2^-1022 and 2^1023, and a factor 2 (sigma), 4 (Sigma, var) commutes with every rounding.
(c) exact       sigma_x0 = 0: var == 0 at step 0, z = +inf (or -inf for a plan inside the margin); a sphere on the base link: var == 0 at every
                step; a self pair moved by the same joints: exact zeros; ties to the lowest (i, j); a duplicated obstacle ties exactly.
(d) bad inputs  a NaN / inf joint position planted in the plan: NaN entries, clr_z_at = (k0, -1, -1), not eligible; the other plans on bytes.
(e) selection   ilqr_problem_select with the call's `eligible`: five groups of three hand-written starts, one group without an eligible start.
(f) untouched   X, U, K, d, cost, lambda, status, the plan / gains flags and the problem's own obstacle terms.
(g) refusals    each by its text.
(i) meaning     PosOrn-1: the sample variance of a plane pair's clearance over 4096 executions lies in the chi-square 1e-6 interval about clr_var."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ilqr_planner_amd import capi, workloads
from tests import clearance as clr
from tests import clearance_reference as cref
from tests import closed_loop as cl
from tests import cov_clearance_reference as ref
from tests import multistart as ms
from tests import obstacles as ob
from tests import self_collision as sc

MARGIN = 0.05
Z_TOL = 3.0
SIGMA_W, SIGMA_X0 = 1e-3, 4e-3
#       name: (chain, system, B, T, spheres, obstacles, planes, traj_per_set or None for B, pairs, anchors, iterations, fd_every)
CASES = {
    "one": ("panda", "po1", 1, 2, 1, 1, 0, 1, 0, 0, 0, 1),
    "gen4": ("gen4", "pot2", 13, 3, 5, 9, 2, 1, 7, 3, 3, 1),
    "gen7": ("gen7", "po2", 70, 2, 5, 1, 0, 5, 1, 1, 0, 7),
    "wall": ("panda", "po1", 13, 9, 5, 9, 2, None, 0, 0, 3, 5),
    "long": ("panda", "js1", 1, 9, 32, 9, 2, None, 7, 3, 3, 1),
}
# chosen on the reference alone: the reference's own gap assertions hold
SEED = {"one": 0, "gen4": 0, "gen7": 0, "wall": 0, "long": 0}


def sigmas(p, scale=1.0):
    """sigma_w, sigma_x0 in the user's state layout: every entry its own value, so that no two rows of Sigma are alike."""
    n = p.dims.n_x
    return scale * SIGMA_W * (1.0 + 0.1 * np.arange(n)), scale * SIGMA_X0 * (1.0 + 0.05 * np.arange(n))


def plan(p, nit):
    """A plan with gains: a 3-iteration solve, or the rollout of the controls as they are with ilqr_problem_gains about it."""
    p.solve_recursive(nit, True, False)
    if nit == 0:
        p.gains()


def build(ctx, name):
    """(desc, inp, chain, spheres, planes, obs or None, traj_per_set, pairs, nit, fd_every) of a case."""
    cname, system, B, T, n_sph, n_obs, n_pl, tps, n_pairs, n_anchor, nit, fd = CASES[name]
    rng = np.random.default_rng(6000 + SEED[name] + sum(map(ord, name)))
    cfg, desc, inp, chain = ob.make_problem(ctx, cname, system, T, B, u_scale=0.2)
    tps = B if tps is None else tps
    if n_pairs:
        sph, pairs = sc.robot_of(chain, n_sph, n_pairs, n_anchor, rng)
    else:
        sph, pairs = clr.spheres_of(chain, n_sph, rng), []
    obs = clr.obstacles_of(B // tps, n_obs, rng) if n_obs else None
    return desc, inp, chain, sph, clr.planes_of(n_pl), obs, tps, pairs, nit, fd


def world_of(obs, tps, margin):
    return (obs, tps, margin)


def call_dev(p, arrays, sw, sx, rb, obs, tps, margin, z_tol, with_Sigma=False):
    """The _dev form on the arrays of the runner; returns a ClosedLoopCovClr (Sigma where asked for, the other covariance outputs None)."""
    B, T, nx = p.B, p.T, p.dims.n_x
    obs = np.zeros((B // tps, 0, 4)) if obs is None else obs
    ho = arrays.put(obs)
    w = capi.ClrWorld(arrays.ptr(ho) if obs.size else None, obs.shape[0], obs.shape[1], int(tps), float(margin), 0)
    hs = [arrays.empty((B, T)), arrays.empty((B, T)), arrays.empty(B), arrays.empty((B, 3), np.int32), arrays.empty(B, np.int32)]
    hS = arrays.empty((B, T, nx, nx)) if with_Sigma else None
    cov = capi.Cov(arrays.ptr(hS), None, None, None, None) if with_Sigma else None
    p.closed_loop_cov_clr_dev(sw, sx, rb, w, z_tol, capi.ClCovClr(*(arrays.ptr(h) for h in hs)), cov)
    p.ctx.synchronize()
    got = [np.array(arrays.get(h)) for h in hs]
    return capi.ClosedLoopCovClr(np.array(arrays.get(hS)) if with_Sigma else None, None, None, None, None, *got)


def same(a, b, tag, fields=capi.COV_CLR_OUTPUTS):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert x.tobytes() == y.tobytes(), f"{tag}: {f} differs ({int(np.sum(x != y))} entries, NaN counted)"


def against_reference(got, r, tag):
    """Returns the worst |error| / bound of clr_var and of clr_z."""
    worst = dict(var=0.0, z=0.0)
    for f, bound, key in (("clr_var", r["var_bound"], "var"), ("clr_z", r["z_bound"], "z"), ("clr_z_min", r["z_min_bound"], "z")):
        g, e = getattr(got, f), r[f]
        assert np.array_equal(np.isnan(g), np.isnan(e)), f"{tag}: {f}: NaN pattern"
        inf = np.isinf(e)
        assert np.array_equal(g[inf], e[inf]) and not np.any(np.isinf(g[~inf & ~np.isnan(e)])), f"{tag}: {f}: the infinities differ"
        ok = np.isfinite(e)
        err = np.abs(g[ok] - e[ok])
        exact = bound[ok] == 0
        assert np.all(err[exact] == 0), f"{tag}: {f}: an entry the reference has exactly is {err[exact].max():.3e} off"
        ratio = float(np.max(err[~exact] / bound[ok][~exact], initial=0.0))
        print(f"{tag}: {f}: worst |error| / bound {ratio:.3e}", flush=True)
        assert ratio <= 1.0, f"{tag}: {f} is {ratio:.3e} bounds from the 50-digit reference"
        worst[key] = max(worst[key], ratio)
    assert np.array_equal(got.clr_z_at, r["clr_z_at"]), f"{tag}: clr_z_at {got.clr_z_at[np.any(got.clr_z_at != r['clr_z_at'], axis=1)][:4]} against the reference"
    assert np.array_equal(got.eligible, r["eligible"]), f"{tag}: eligible"
    return worst


_REF = {}


# ------------------------------------------------------------------------------------------------ (a) values, (b) bit rules

def check_values(ctx, arrays, name, pin=True):
    """(a) and (b) of one case under one pin.  Returns the worst ratios to the bounds."""
    desc, inp, chain, sph, pl, obs, tps, pairs, nit, fd = build(ctx, name)
    B, dof = len(inp["q0"]), chain["dof"]
    tag = f"{name} {'generic' if pin else 'rows'}"
    rb = capi.clr_robot(sph, pl, self_pairs=pairs)
    p = workloads.load_batch(ctx, desc, inp, B)
    try:
        with ob.generic_pin(pin):
            plan(p, nit)
            sw, sx = sigmas(p)
            before = p.closed_loop_cov(sw, sx, want_Sigma=True)
            got = p.closed_loop_cov_clr(sw, sx, rb, world_of(obs, tps, MARGIN), Z_TOL, want=capi.COV_CLR_OUTPUTS + ("Sigma", "kp_Sigma", "kp_var", "u_var", "lim_z"))
            for f in capi.ClosedLoopCov._fields:   # `out` on the bytes of closed_loop_cov under the same pin
                assert getattr(got, f).tobytes() == getattr(before, f).tobytes(), f"{tag}: {f} differs from closed_loop_cov's"
            after = p.closed_loop_cov(sw, sx, want_Sigma=True)
            for f in capi.ClosedLoopCov._fields:
                assert getattr(after, f).tobytes() == getattr(before, f).tobytes(), f"{tag}: closed_loop_cov's {f} moved over a _clr call"
            key = (name, pin)
            Q = p.X()[..., :dof]
            if key not in _REF:
                _REF[key] = (Q.copy(), got.Sigma.copy(), ref.cov_clearance(chain, Q, got.Sigma, sph, pl, obs, pairs, tps, MARGIN, Z_TOL, fd_every=fd))
            assert _REF[key][0].tobytes() == Q.tobytes() and _REF[key][1].tobytes() == got.Sigma.tobytes(), f"{tag}: the plan or Sigma differs from the reference's"
            r = _REF[key][2]
            print(f"{tag}: the reference's smallest gap is {float(r['worst_gap']):.3e} times 1000 bounds", flush=True)
            worst = against_reference(got, r, tag)
            assert np.any(got.clr_z_at[:, 1] >= 0) and np.all(got.clr_var[np.isfinite(got.clr_z)] > 0), f"{tag}: the case shows nothing"
            # without `out`, a subset, and the _dev form (Sigma in the context's buffer, and in the caller's)
            alone = p.closed_loop_cov_clr(sw, sx, rb, world_of(obs, tps, MARGIN), Z_TOL)
            same(alone, got, f"{tag}: without out")
            assert alone.Sigma is None and alone.lim_z is None
            only = p.closed_loop_cov_clr(sw, sx, rb, world_of(obs, tps, MARGIN), Z_TOL, want=("clr_z_min", "lim_z"))
            assert only.clr_z is None and only.clr_z_min.tobytes() == got.clr_z_min.tobytes() and only.lim_z.tobytes() == got.lim_z.tobytes()
            same(call_dev(p, arrays, sw, sx, rb, obs, tps, MARGIN, Z_TOL), got, f"{tag}: _dev form")
            dv = call_dev(p, arrays, sw, sx, rb, obs, tps, MARGIN, Z_TOL, with_Sigma=True)
            same(dv, got, f"{tag}: _dev form with Sigma")
            assert dv.Sigma.tobytes() == got.Sigma.tobytes(), f"{tag}: Sigma of the _dev form"
            # sigmas times 2
            sw2, sx2 = sigmas(p, 2.0)
            twice = p.closed_loop_cov_clr(sw2, sx2, rb, world_of(obs, tps, MARGIN), Z_TOL)
            assert twice.clr_var.tobytes() == (4.0 * got.clr_var).tobytes(), f"{tag}: sigmas times 2: clr_var is not 4 times the original bit for bit"
            assert twice.clr_z.tobytes() == (0.5 * got.clr_z).tobytes(), f"{tag}: sigmas times 2: clr_z is not half the original bit for bit"
            assert np.array_equal(twice.clr_z_at, got.clr_z_at), f"{tag}: sigmas times 2: clr_z_at moved"
        return worst
    finally:
        p.close()


def check_cov_con_unchanged(ctx, pin=True, tag="cov_con"):
    """ilqr_problem_closed_loop_cov_con is byte-equal to itself before and after a _clr call."""
    T, B = 9, 13
    cfg, desc, inp = ms.make_case(ctx, "C3", T, B)
    chain = clr.chain_of("panda0")
    sph = clr.spheres_of(chain, 5, np.random.default_rng(2))
    p = workloads.load_batch(ctx, desc, inp, B)
    try:
        with ob.generic_pin(pin):
            p.set_constraints(inp["A"], inp["b"], inp["lambda0"])
            ms.solve(p, cfg, 3)
            sw, sx = sigmas(p)
            a = p.closed_loop_cov_con(sw, sx, want_Sigma=True, want_lim_z=True)
            got = p.closed_loop_cov_clr(sw, sx, capi.clr_robot(sph, clr.planes_of(2)), world_of(None, B, MARGIN), Z_TOL)
            assert np.all(np.isfinite(got.clr_z_min))
            b = p.closed_loop_cov_con(sw, sx, want_Sigma=True, want_lim_z=True)
            for f in ("Sigma", "lim_z", "con_var", "con_z"):
                assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f"{tag}: {f} moved over a _clr call"
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (c) exact cases

def check_exact(ctx, arrays, pin=True, tag="exact"):
    T, B = 3, 13
    cfg, desc, inp, chain = ob.make_problem(ctx, "panda", "po1", T, B, u_scale=0.2)
    n_seg = len(chain["seg_joint"])
    tool = n_seg - 1
    seg = [s for s, j in enumerate(chain["seg_joint"]) if int(j) >= 0]
    p = workloads.load_batch(ctx, desc, inp, B)
    try:
        with ob.generic_pin(pin):
            plan(p, 0)
            sw, sx = sigmas(p)
            X = p.X()
            far = np.array([[[5.0, 5.0, 5.0, 0.1]]])
            # sigma_x0 = 0: Sigma_0 = 0, so every pair has var == 0 at step 0: +inf for a plan clear of the margin ...
            rb = capi.clr_robot([(tool, (0.0, 0.0, 0.05), 0.02)])
            got = p.closed_loop_cov_clr(sw, None, rb, world_of(far, B, MARGIN), Z_TOL)
            assert np.all(got.clr_z[:, 0] == np.inf) and np.all(got.clr_var[:, 0] == 0.0), f"{tag}: sigma_x0 = 0: step 0 is {got.clr_z[:, 0]}"
            assert np.all(np.isfinite(got.clr_z[:, 1:])) and np.all(got.clr_var[:, 1:] > 0) and np.all(got.clr_z_at[:, 0] >= 1)
            # ... and -inf for a plan planted inside it: an obstacle around the tool sphere's place at step 0
            R_, p_ = cref.link_frames(chain, X[0, 0, :7], tool)[tool + 1]
            c = p_ + R_ * cref.mp.matrix([0.0, 0.0, 0.05])
            inside = np.empty((B, 1, 4))
            for b in range(B):   # a set per plan
                Rb, pb = cref.link_frames(chain, X[b, 0, :7], tool)[tool + 1]
                cb = pb + Rb * cref.mp.matrix([0.0, 0.0, 0.05])
                inside[b, 0] = (float(cb[0]) + 0.01, float(cb[1]), float(cb[2]), 0.1)
            got = p.closed_loop_cov_clr(sw, None, rb, world_of(inside, 1, MARGIN), Z_TOL)
            assert np.all(got.clr_z[:, 0] == -np.inf) and np.all(got.clr_var[:, 0] == 0.0), f"{tag}: inside the margin at step 0: {got.clr_z[:, 0]}"
            assert np.all(got.clr_z_min == -np.inf) and np.all(got.clr_z_at == (0, 0, 0)) and np.all(got.eligible == 0)
            # a sphere on the base link: var == 0 at every step
            rb = capi.clr_robot([(-1, (0.1, 0.0, 0.3), 0.05)], clr.planes_of(2))
            got = p.closed_loop_cov_clr(sw, sx, rb, world_of(None, B, MARGIN), Z_TOL)
            assert np.all(got.clr_var == 0.0) and np.all(got.clr_z == np.inf) and np.all(got.clr_z_min == np.inf), f"{tag}: a sphere on the base link"
            assert np.all(got.clr_z_at == (0, -1, -1)) and np.all(got.eligible == 1)
            below = p.closed_loop_cov_clr(sw, sx, capi.clr_robot([(-1, (0.1, 0.0, -0.3), 0.05)], clr.planes_of(1)), world_of(None, B, MARGIN), Z_TOL)
            assert np.all(below.clr_z == -np.inf) and np.all(below.clr_z_at == (0, 0, 0)) and np.all(below.eligible == 0), f"{tag}: a base sphere under the floor"
            # a self pair between the links behind joints 1 and 2: only joint 2 moves one sphere and not the other.  Sigma_0 = diag(sigma_x0^2), so at
            # step 0 a start spread on joint 2 alone gives the pair a variance, and a spread on every other joint gives exactly 0
            rb = capi.clr_robot([(seg[1], (0.02, 0.0, 0.0), 0.01), (seg[2], (0.0, 0.03, 0.1), 0.01)], self_pairs=[(0, 1)])
            only2 = np.zeros(p.dims.n_x)
            only2[2] = 1e-3
            rest = np.full(p.dims.n_x, 1e-3)
            rest[2] = 0.0
            hit = p.closed_loop_cov_clr(None, only2, rb, world_of(None, B, 0.0), Z_TOL)
            assert np.all(hit.clr_var[:, 0] > 0), f"{tag}: the joint between the pair's links gives no variance"
            miss = p.closed_loop_cov_clr(None, rest, rb, world_of(None, B, 0.0), Z_TOL)
            assert np.all(miss.clr_var[:, 0] == 0.0) and np.all(np.isinf(miss.clr_z[:, 0])), f"{tag}: joints that move both spheres give {miss.clr_var[:, 0]}"
            # ties: two spheres in one place, and a duplicated obstacle: the lowest (i, j)
            near = np.array([float(c[0]) + 0.3, float(c[1]), float(c[2]), 0.05])
            obs = np.array([[[5.0, 5.0, 5.0, 0.1], near, near]])
            rb = capi.clr_robot([(-1, (0.0, 0.0, 0.0), 0.01), (tool, (0.0, 0.0, 0.05), 0.02), (tool, (0.0, 0.0, 0.05), 0.02)])
            got = p.closed_loop_cov_clr(sw, sx, rb, world_of(obs, B, MARGIN), Z_TOL)
            r = ref.cov_clearance(chain, X[..., :7], p.closed_loop_cov(sw, sx, want_Sigma=True).Sigma, [(-1, (0.0, 0.0, 0.0), 0.01), (tool, (0.0, 0.0, 0.05), 0.02),
                                  (tool, (0.0, 0.0, 0.05), 0.02)], [], obs, [], B, MARGIN, Z_TOL, ties=True)
            assert np.all(r["clr_z_at"][:, 1:] == (1, 1)), f"{tag}: the case does not put its minimum on the doubled pair: {r['clr_z_at']}"
            assert np.array_equal(got.clr_z_at, r["clr_z_at"]), f"{tag}: ties: clr_z_at {got.clr_z_at}"
            one = p.closed_loop_cov_clr(sw, sx, capi.clr_robot([(tool, (0.0, 0.0, 0.05), 0.02)]), world_of(obs[:, 1:2], B, MARGIN), Z_TOL)
            assert one.clr_z.tobytes() == got.clr_z.tobytes() and one.clr_var.tobytes() == got.clr_var.tobytes(), f"{tag}: the duplicates do not tie exactly"
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (d) bad inputs

def check_bad(ctx, arrays, pin=True, tag="bad"):
    """A NaN planted in plan 3's joint positions at step 1 (through its first control) and an inf in plan 7's at step 0 (through its initial
    state).  The gains about a plan that is not finite are not finite either, so from step 1 on such a plan's Sigma_k is bad as well: the first
    bad step is the planted one in both."""
    T, B = 9, 13
    cfg, desc, inp, chain = ob.make_problem(ctx, "panda", "po1", T, B, u_scale=0.2)
    sph = clr.spheres_of(chain, 5, np.random.default_rng(8))
    rb = capi.clr_robot(sph, clr.planes_of(2))
    p, q = workloads.load_batch(ctx, desc, inp, B), workloads.load_batch(ctx, desc, inp, B)
    try:
        with ob.generic_pin(pin):
            plan(p, 0)
            sw, sx = sigmas(p)
            good = p.closed_loop_cov_clr(sw, sx, rb, world_of(None, B, MARGIN), Z_TOL)
            U, q0 = inp["U0"].copy(), np.array(inp["q0"], float)
            U[3, 0, 0] = np.nan
            q0[7, 1] = np.inf
            q.set_init_state(q0)
            q.set_controls(U)
            plan(q, 0)
            X = q.X()
            assert np.all(np.isfinite(X[3, 0])) and np.isnan(X[3, 1, 0]) and np.isinf(X[7, 0, 1]), f"{tag}: the plant is not where it is meant"
            got = q.closed_loop_cov_clr(sw, sx, rb, world_of(None, B, MARGIN), Z_TOL)
            for b, k0 in ((3, 1), (7, 0)):
                assert np.all(np.isnan(got.clr_z[b, k0:])) and np.all(np.isnan(got.clr_var[b, k0:])) and np.isnan(got.clr_z_min[b]), f"{tag}: plan {b}: {got.clr_z[b]}"
                assert np.all(np.isfinite(got.clr_z[b, :k0])), f"{tag}: plan {b}: a step before the plant is bad"
                assert tuple(got.clr_z_at[b]) == (k0, -1, -1) and got.eligible[b] == 0, f"{tag}: plan {b}: clr_z_at {got.clr_z_at[b]}"
            rest = [b for b in range(B) if b not in (3, 7)]
            for f in capi.COV_CLR_OUTPUTS:
                assert getattr(got, f)[rest].tobytes() == getattr(good, f)[rest].tobytes(), f"{tag}: {f} of an untouched plan moved"
    finally:
        p.close()
        q.close()


# ------------------------------------------------------------------------------------------------ (e) selection

def check_selection(ctx, arrays, pin=True, tag="selection"):
    """Five groups of three hand-written starts, each start with an obstacle set of its own: far away, or 1 mm beyond the margin of the tool
    sphere's last position for the starts meant to fail z_tol.  Group 3 has no start that keeps z_tol: member 0 wins."""
    G, S, T = 5, 3, 9
    B = G * S
    cfg, desc, inp, p = clr.make_problem(ctx, "panda", "po1", T, B, random_controls=False)
    chain = clr.chain_of("panda")
    tool = len(chain["seg_joint"]) - 1
    for b in range(B):   # member s of group g turns joint s + 1 at its own rate
        inp["U0"][b, :, (b % S) + 1] = 0.2 + 0.05 * (b // S) + 0.1 * (b % S)
        inp["U0"][b, :, 0] = -0.1 * (1 + b % S)
    try:
        with ob.generic_pin(pin):
            p.set_controls(inp["U0"])
            plan(p, 0)
            X, cost, status = p.X(), p.cost(), p.status()
            order = [sorted(range(g * S, (g + 1) * S), key=lambda b: cost[b]) for g in range(G)]
            blocked = {0: [], 1: order[1][:1], 2: order[2][:2], 3: order[3], 4: [4 * S]}
            members = [b for g in range(G) for b in blocked[g]]
            sph = [(tool, (0.0, 0.0, 0.05), 0.02)]
            obs = np.tile(np.array([5.0, 5.0, 5.0, 0.1]), (B, 1, 1))
            for b in members:
                R_, p_ = cref.link_frames(chain, X[b, T - 1, :7], tool)[tool + 1]
                c = p_ + R_ * cref.mp.matrix([0.0, 0.0, 0.05])
                obs[b, 0] = (float(c[0]), float(c[1]), float(c[2]) + 0.02 + 0.1 + MARGIN + 1e-3, 0.1)   # clearance margin + 1 mm at the last step
            sw, sx = sigmas(p)
            rb = capi.clr_robot(sph)
            got = p.closed_loop_cov_clr(sw, sx, rb, world_of(obs, 1, MARGIN), Z_TOL, want=capi.COV_CLR_OUTPUTS + ("Sigma",))
            r = ref.cov_clearance(chain, X[..., :7], got.Sigma, sph, [], obs, [], 1, MARGIN, Z_TOL, fd_every=9)
            expect = np.ones(B, np.int32)
            expect[members] = 0
            assert np.array_equal(r["eligible"], expect), f"{tag}: below z_tol {np.flatnonzero(r['eligible'] == 0)}, meant {np.flatnonzero(expect == 0)} (z_min {r['clr_z_min']})"
            against_reference(got, r, tag)
            sel = p.select(S, None, got.eligible)
            ms.same_selection(sel, ms.select_ref(cost, got.eligible, status, S), tag)
            for g in range(G):
                keep = [b for b in order[g] if expect[b]]
                assert sel.winner[g] == (keep[0] if keep else g * S) and sel.n_candidates[g] == len(keep), f"{tag}: group {g}: winner {sel.winner[g]}, {sel.n_candidates[g]} candidates"
            assert sel.n_candidates[3] == 0 and sel.winner[3] == 3 * S
            dv = call_dev(p, arrays, sw, sx, rb, obs, 1, MARGIN, Z_TOL)
            assert dv.eligible.tobytes() == got.eligible.tobytes(), f"{tag}: eligible of the _dev form"
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (f) untouched state

def check_untouched(ctx, arrays, pin=True, tag="untouched"):
    T, B = 9, 13
    cfg, desc, inp = ms.make_case(ctx, "C3", T, B)
    chain = clr.chain_of("panda0")
    rng = np.random.default_rng(4)
    sph = clr.spheres_of(chain, 5, rng)
    own = clr.obstacles_of(B, 3, rng)   # the problem's own obstacle terms: another geometry than the call's
    p = workloads.load_batch(ctx, desc, inp, B)
    try:
        with ob.generic_pin(pin):
            p.set_constraints(inp["A"], inp["b"], inp["lambda0"])
            p.set_obstacles(sph[:2], [], own, 0.3, 5.0, 1)
            ms.solve(p, cfg, 3)
            snap = lambda: dict(X=p.X(), U=p.U(), K=p.K(), d=p.d(), cost=p.cost(), lam=p.lam(), status=p.status(), iters=p.iters(), alpha=p.alpha(),   # noqa: E731
                                **{"obs_" + k: v for k, v in p.obstacle_terms()._asdict().items()})
            before = snap()
            sw, sx = sigmas(p)
            got = p.closed_loop_cov_clr(sw, sx, capi.clr_robot(sph, clr.planes_of(2)), world_of(clr.obstacles_of(1, 9, rng), B, MARGIN), Z_TOL)
            call_dev(p, arrays, sw, sx, capi.clr_robot(sph, clr.planes_of(2)), None, B, MARGIN, Z_TOL)
            assert not np.any(np.isnan(got.clr_z_min))
            after = snap()
            for k, v in before.items():
                assert v.tobytes() == after[k].tobytes(), f"{tag}: {k} moved"
            # the flags: the calls that need gains and a plan still run
            p.closed_loop_cov(sw, sx)
            p.clearance(capi.clr_robot(sph, clr.planes_of(2)), None, B, MARGIN)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (g) refusals

def check_refusals(ctx, arrays, tag="refusals"):
    desc, inp, chain, sph, pl, obs, tps, pairs, nit, fd = build(ctx, "gen4")
    B = len(inp["q0"])
    p = workloads.load_batch(ctx, desc, inp, B)
    L = ctx.L
    R = cl._refused
    fn = "ilqr_problem_closed_loop_cov_clr"
    zmin = np.empty(B)
    sig = np.full(p.dims.n_x, 1e-3)

    def call(rb=None, n_obs=None, z_tol=Z_TOL, clr_out=True, out=None, sw=sig, margin=MARGIN, tps_=tps, world=True, name=fn):
        rb = capi.clr_robot(sph, pl, self_pairs=pairs) if rb is None else rb
        w = capi.ClrWorld(obs.ctypes.data, obs.shape[0], obs.shape[1] if n_obs is None else n_obs, tps_, margin, 0)
        ck = capi.ClCovClr(None, None, zmin.ctypes.data if clr_out else None, None, None)
        ctx.check(getattr(L, name)(p.h, capi._dp(sw), None, C.byref(out) if out is not None else None, C.byref(rb) if rb is not False else None,
                                   C.byref(w) if world else None, float(z_tol), C.byref(ck) if clr_out is not None else None))

    try:
        R(lambda: call(), "closed loop needs the gains")
        plan(p, nit)
        call()   # the base call is accepted, a NULL out included
        bad = sig.copy()
        bad[0] = -1.0
        R(lambda: call(sw=bad), "every sigma_w and sigma_x0 must be finite and >= 0")
        R(lambda: call(rb=False), f"{fn}: robot is a null pointer")
        R(lambda: call(world=False), f"{fn}: world is a null pointer")
        R(lambda: call(name=fn + "_dev", world=False), f"{fn}_dev: world is a null pointer")
        rb = capi.clr_robot(sph, pl, self_pairs=pairs)
        rb.n_sph = 33
        R(lambda: call(rb=rb), f"{fn}: n_sph must be 1 .. 32 (got 33)")
        R(lambda: call(rb=capi.clr_robot(sph, pl, self_pairs=[(2, 1)])), f"{fn}: self_pair[0] = (2, 1) must have a < b")
        R(lambda: call(rb=capi.clr_robot(sph, [((0.0, 0.0, 2.0), 0.0)])), f"{fn}: plane_n[0] is not a unit vector")
        R(lambda: call(n_obs=-1), f"{fn}: n_obs must be >= 0 (got -1)")
        R(lambda: call(tps_=2), f"{fn}: the number of trajectories ({B}) is not a multiple of traj_per_set (2)")
        R(lambda: call(rb=capi.clr_robot(sph), n_obs=0), f"{fn}: nothing to keep clear of: n_obs = 0 and n_planes = 0")
        R(lambda: call(margin=np.nan), f"{fn}: margin is NaN")
        R(lambda: call(z_tol=np.nan), f"{fn}: z_tol is NaN")
        R(lambda: call(clr_out=False), f"{fn}: clr and out both ask for nothing")
        R(lambda: call(clr_out=None), f"{fn}: clr and out both ask for nothing")
        R(lambda: call(clr_out=False, out=capi.Cov(None, None, None, None, None)), f"{fn}: clr and out both ask for nothing")
        lim = np.empty(B)
        call(clr_out=False, out=capi.Cov(None, None, None, None, lim.ctypes.data))   # `out` alone is a covariance call
        assert lim.tobytes() == p.closed_loop_cov(sig, None, want_kp_Sigma=False, want_kp_var=False, want_u_var=False).lim_z.tobytes()
        nochain = ms.make_case(ctx, "C1j", 3, 2)
        pj = workloads.load_batch(ctx, nochain[1], nochain[2], 2)
        try:
            plan(pj, 0)
            R(lambda: pj.closed_loop_cov_clr(1e-3, None, capi.clr_robot(sph, pl), world_of(None, 2, MARGIN), Z_TOL), f"{fn}: the descriptor has no chain")
        finally:
            pj.close()
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (i) meaning

def check_meaning(ctx, arrays, pin=True, tag="meaning"):
    """PosOrn-1, one plan, one tool sphere above the floor: the sample variance of the plane pair's clearance over S = 4096 executions of
    closed_loop_noise, at the step clr_z_at names, against clr_var."""
    T, S = 9, 4096
    cfg, desc, inp, chain = ob.make_problem(ctx, "panda", "po1", T, 1, u_scale=0.2)
    tool = len(chain["seg_joint"]) - 1
    sphere, plane = (tool, (0.0, 0.0, 0.05), 0.02), ((0.0, 0.0, 1.0), -0.5)
    rb = capi.clr_robot([sphere], [plane])
    p = workloads.load_batch(ctx, desc, inp, 1)
    try:
        with ob.generic_pin(pin):
            plan(p, 3)
            sw, sx = sigmas(p)
            sx = 0.05 * sx   # the spread grows along the plan: the minimum in z lies behind step 0, where Sigma_k carries the recursion
            got = p.closed_loop_cov_clr(sw, sx, rb, world_of(None, 1, MARGIN), Z_TOL, want=capi.COV_CLR_OUTPUTS + ("Sigma",))
            k, i, j = (int(v) for v in got.clr_z_at[0])
            assert (i, j) == (0, 0) and k >= 1, f"{tag}: clr_z_at {got.clr_z_at[0]}"
            lo, hi = ref.chi2_interval(S - 1, 1e-6)
            share, var1 = ref.curvature_share(chain, p.X()[0, k], got.Sigma[0, k], sphere, plane)
            half = float(min(1 - lo, hi - 1))
            print(f"{tag}: chi-square interval [{float(lo):.5f}, {float(hi):.5f}] of the variance; curvature adds {float(share):.3e} of it", flush=True)
            assert float(share) <= 0.1 * half, f"{tag}: the curvature of FK adds {float(share):.3e} of the variance (> a tenth of {half:.3e}): choose smaller sigmas"
            assert abs(float(var1) - got.clr_var[0, k]) <= 1e-12 * float(var1) * 49
            ex = p.closed_loop_noise(S, 20261021, sw, sx, want_X=True, want_U=False)
            c = ctx.clearance_trajectories(desc, ex.X.reshape(S, T, -1), rb, None, S, MARGIN, want=("clr",)).clr[:, k]
            s2 = float(np.var(c, ddof=1))
            ratio = s2 / got.clr_var[0, k]
            print(f"{tag}: step {k}: sample variance {s2:.6e}, clr_var {got.clr_var[0, k]:.6e}, ratio {ratio:.5f}", flush=True)
            assert float(lo) <= ratio <= float(hi), f"{tag}: the sample variance is {ratio:.5f} of clr_var, outside [{float(lo):.5f}, {float(hi):.5f}]"
    finally:
        p.close()
