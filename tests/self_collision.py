"""Self-collision pairs in the clearance calls and the obstacle terms (ilqr_clr_robot::n_self / self_pair) -- cases and checks shared by
tests/tools/hostsim/self_collision_checks.py (the host build) and tests/test_gpu_self_collision.py (the device kernels).  The problems, worlds and
helpers are those of tests/clearance.py, tests/obstacles.py and tests/obstacles_coop.py; the references are tests/self_collision_reference.py.

Shapes: T = 2, 3, 9; B = 1, 13, 70 (a wave is crossed); the Panda with a tool frame, gen7 and gen4 (four joints: the padded joints must get
nothing); PosOrn-1, PosOrn-2, PosOrnTime-2 and JointSpace-1 with a chain; 5 and 32 spheres; 1, 7 and 64 pairs on 1, 3 and 8 anchors, with an anchor
on link -1, one on a fixed segment, a second member on the tool segment and a radius 0; 9 obstacles and 2 planes, or no world at all;
traj_per_set 1 and B.

(a) clearance   clr, clr_min within 1e-12 of the 50-digit reference, clr_at (the self code n_obs + n_planes + a included), n_below and eligible
                exactly; host and _dev form; a duplicated anchor ties to the lower a; a planted NaN is a bad step; the problem form against the
                trajectory form on bytes.
(b) terms       obstacle_terms() within 1e-12 max(1, w) max(1, |ref|); lxx exactly symmetric; with self pairs alone, the entries of the joints
                before the first anchor's link and behind the last second member's link == 0.0; the reference's l_x against the central difference.
(c) inert       n_self = 0 through the keyword gives the bytes of the call without it; pairs that stay beyond the margin give the solve without
                them on bytes; after clear_obstacles() the bytes of a problem that never had terms.
(d) iterations  one and three iterations of the recursive and the AL solve against the float64 restatement: K, d at K_TOL / D_TOL of
                tests/gains.py, cost at rtol 1e-9, step sizes and iteration counts exactly.  On a context in cooperative mode the same, and one
                iteration of generic against cooperative mode at K_TOL / D_TOL.
(e) bite        a plan whose tool sphere runs through a sphere on the base: on the reference alone clr_min < 0 without the term and >= margin / 2
                with it; the library's plans, scored by ilqr_problem_clearance, are held to that.
(f) multi-start five groups of three hand-written starts, chosen members in self-collision: select with the call's `eligible`.
(g) gains       gains() / gains_al() about a self-collision plan: K of a fresh one-iteration solve on bytes, d alpha times it.
(h) refusals    each by its text."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ilqr_planner_amd import capi, workloads
from tests import clearance as clr
from tests import clearance_reference as cref
from tests import closed_loop as cl
from tests import multistart as ms
from tests import obstacle_reference as oref
from tests import obstacles as ob
from tests import obstacles_coop as oc
from tests import self_collision_reference as ref
from tests.gains import D_TOL, K_TOL

TOL = 1e-12
MARGIN = 0.4   # wide enough that neighbouring links' spheres are within it
CASE_MARGIN = {"one": 1.0, "inner": 1.0}   # few pairs: a margin that reaches across the arm, so that they are active at every state
#       name: (chain, system, B, T, spheres, obstacles, planes, traj_per_set or None for B, pairs, anchors, inner, weight)
#       inner: hand-placed spheres, the pairs between the second and the fifth joint, so that joints at both ends of the chain move no pair
CASES = {
    "one": ("panda", "po1", 1, 2, 5, 0, 0, 1, 1, 1, False, 50.0),
    "gen4": ("gen4", "pot2", 13, 3, 5, 9, 2, 1, 7, 3, False, 0.5),
    "gen7": ("gen7", "po2", 70, 2, 5, 0, 0, None, 7, 3, False, 3.0),
    "inner": ("gen7", "po1", 13, 3, 5, 0, 0, None, 2, 1, True, 200.0),
    "long": ("panda", "js1", 1, 9, 32, 9, 2, None, 64, 8, False, 7.0),
}
#           name: (chain, system, n, T, spheres, obstacles, planes, traj_per_set or None for n, pairs, anchors)
CLR_CASES = {
    "one": ("panda", "po1", 1, 2, 5, 0, 0, 1, 1, 1),
    "gen4": ("gen4", "pot2", 13, 3, 5, 9, 2, 1, 7, 3),
    "gen7": ("gen7", "po1", 70, 2, 5, 0, 0, None, 7, 3),
    "long": ("panda", "po1", 1, 9, 32, 9, 2, None, 64, 8),
    "po2": ("gen7", "po2", 13, 3, 5, 9, 2, None, 7, 3),
    "js1": ("panda", "js1", 13, 2, 5, 0, 0, 1, 7, 3),
}
# chosen on the reference alone: the spheres give the wanted pairs and anchors, the reference's own gaps hold, and self pairs are minima
CLR_SEED = {"one": 3000, "gen4": 3008, "gen7": 3001, "long": 3018, "po2": 3001, "js1": 3000}


def clr_desc_of(chain, system, T):
    """clearance.desc_of for every system of tests/obstacles.SYSTEMS: of the descriptor only kind, nb_deriv, dof and the chain are read."""
    kind, nd, _ = ob.SYSTEMS[system]
    return capi.make_desc(kind=kind, nb_deriv=nd, horizon=max(T, 2), dt=0.05, R_diag=[1e-5] * 8, chain=chain, kp_timesteps=[], kp_Q=[])


def clr_states_of(n, T, chain, system, rng):
    """clearance.states_of for the same systems: joint positions in -2.5 .. 2.5 first, anything behind them."""
    kind, nd, _ = ob.SYSTEMS[system]
    n_x = nd * chain["dof"] + (1 if kind in (capi.SYS_POS_ORN_TIME, capi.SYS_JOINT_TIME) else 0)
    X = rng.normal(0.0, 3.0, (n, T, n_x))
    X[..., : chain["dof"]] = rng.uniform(-2.5, 2.5, (n, T, chain["dof"]))
    return X


def _moves(chain, la, lb):
    return any(int(chain["seg_joint"][s]) >= 0 for s in range(la + 1, lb + 1))


def pairs_of(chain, sph, n_pairs, n_anchor):
    """n_pairs self pairs on n_anchor anchors in no sorted order.  The anchors: the first sphere that has a partner (link -1 where the spheres
    have one), one on a fixed segment where there is one, then the lowest others; the pairs go round the anchors, each anchor's farthest partner
    (the tool's sphere) first."""
    n = len(sph)
    every = [(a, b) for a in range(n) for b in range(a + 1, n) if sph[a][0] < sph[b][0] and _moves(chain, sph[a][0], sph[b][0])]
    cand = sorted({a for a, _ in every})
    fixed = [a for a in cand if sph[a][0] >= 0 and int(chain["seg_joint"][sph[a][0]]) < 0]
    anchors = []
    for a in cand[:1] + fixed[:1] + cand:
        if a not in anchors and len(anchors) < n_anchor:
            anchors.append(a)
    assert len(anchors) == n_anchor, f"the spheres give {len(anchors)} anchors, {n_anchor} wanted"
    per = {a: [p for p in reversed(every) if p[0] == a] for a in anchors}
    out = []
    while len(out) < n_pairs:
        took = False
        for a in anchors:
            if per[a] and len(out) < n_pairs:
                out.append(per[a].pop(0))
                took = True
        assert took, f"the spheres give {len(out)} pairs on these anchors, {n_pairs} wanted"
    return out


def robot_of(chain, n_sph, n_pairs, n_anchor, rng):
    """(spheres, pairs): clearance.spheres_of drawn from rng until the spheres give the wanted pairs and anchors (random links may coincide)."""
    for _ in range(100):
        sph = clr.spheres_of(chain, n_sph, rng)
        try:
            return sph, pairs_of(chain, sph, n_pairs, n_anchor)
        except AssertionError:
            continue
    raise AssertionError(f"no draw of {n_sph} spheres gives {n_pairs} pairs on {n_anchor} anchors")


def joints_upto(chain, link):
    """The number of moving joints on the segments 0 .. link: the index of the first joint behind the link."""
    return sum(1 for s in range(link + 1) if int(chain["seg_joint"][s]) >= 0)


# ------------------------------------------------------------------------------------------------ (a) clearance

def build_clr(name):
    """(chain, desc, X, spheres, planes, obs or None, traj_per_set, pairs) of a clearance case."""
    cname, system, n, T, n_sph, n_obs, n_pl, tps, n_pairs, n_anchor = CLR_CASES[name]
    rng = np.random.default_rng(CLR_SEED[name] + sum(map(ord, name)))
    chain = clr.chain_of(cname)
    tps = n if tps is None else tps
    X = clr_states_of(n, T, chain, system, rng)
    sph, pairs = robot_of(chain, n_sph, n_pairs, n_anchor, rng)
    obs = clr.obstacles_of(n // tps, n_obs, rng) if n_obs else None
    return chain, clr_desc_of(chain, system, T), X, sph, clr.planes_of(n_pl), obs, tps, pairs


_REF = {}


def check_clearance(ctx, arrays, name):
    """Returns the worst |error| / tolerance of clr and clr_min."""
    chain, desc, X, sph, pl, obs, tps, pairs = build_clr(name)
    n, T = X.shape[0], X.shape[1]
    if ("clr", name) not in _REF:
        _REF["clr", name] = ref.clearance(chain, X[..., : chain["dof"]], sph, pl, obs, pairs, tps, MARGIN)
    r = _REF["clr", name]
    base = (0 if obs is None else obs.shape[1]) + len(pl)
    assert np.any(r["step_at"][..., 1] >= base), f"{name}: no step has its minimum on a self pair: the case shows nothing"
    assert np.any(r["clr_at"][:, 2] >= base), f"{name}: no trajectory has its minimum on a self pair"
    rb = capi.clr_robot(sph, pl, self_pairs=pairs)
    got = ctx.clearance_trajectories(desc, X, rb, obs, tps, MARGIN)
    clr.against_reference(got, r, f"{name} host form")
    worst = max(float(np.max(np.abs(getattr(got, f) - r[f]))) for f in ("clr", "clr_min")) / TOL
    dev = clr.trajectories_dev(ctx, arrays, desc, X, rb, obs if obs is not None else np.zeros((n // tps, 0, 4)), tps, MARGIN, None)
    clr.same_outputs(dev, got, f"{name} _dev form against the host form")
    # a planted NaN in a joint before the last sphere's link: a bad step, every other trajectory as it was
    t, k = n - 1, T - 1
    Xb = X.copy()
    Xb[t, k, 0] = np.nan
    bad = ctx.clearance_trajectories(desc, Xb, rb, obs, tps, MARGIN)
    assert np.isnan(bad.clr_min[t]) and np.isnan(bad.clr[t, k]) and tuple(bad.clr_at[t]) == (k, -1, -1) and bad.eligible[t] == 0, f"{name}: bad step: {bad.clr_at[t]}"
    for f in ("clr_min", "clr_at", "n_below", "eligible"):
        assert getattr(bad, f)[:t].tobytes() == getattr(got, f)[:t].tobytes(), f"{name}: {f} of an untouched trajectory moved"
    return worst


def check_duplicate_anchor(ctx, arrays, tag="duplicate anchor"):
    """Two anchors with the same link, centre and radius, both paired with the tool's sphere: the tie goes to the lower a."""
    chain = clr.chain_of("panda")
    tool = len(chain["seg_joint"]) - 1
    sph = [(-1, (0.3, 0.0, 0.4), 0.05), (-1, (0.3, 0.0, 0.4), 0.05), (tool, (0.01, 0.02, 0.03), 0.05)]
    pairs = [(1, 2), (0, 2)]
    X = clr.states_of(13, 3, chain, "po1", np.random.default_rng(17))
    desc = clr.desc_of(chain, "po1", 3)
    obs = np.array([[[5.0, 5.0, 5.0, 0.1]]])
    r = ref.clearance(chain, X[..., :7], sph, [], obs, pairs, 13, 0.0, ties=True)
    assert np.all(r["clr_at"][:, 1:] == (2, 1 + 0)), f"{tag}: the case does not put its minimum on the doubled pair: {r['clr_at']}"
    rb = capi.clr_robot(sph, self_pairs=pairs)
    for got in (ctx.clearance_trajectories(desc, X, rb, obs, 13, 0.0), clr.trajectories_dev(ctx, arrays, desc, X, rb, obs, 13, 0.0, None)):
        assert np.array_equal(got.clr_at, r["clr_at"]), f"{tag}: clr_at {got.clr_at} (the lower anchor)"
        assert np.max(np.abs(got.clr_min - r["clr_min"])) <= TOL


def check_forms(ctx, arrays, cname, system, T, B, tps, n_sph, n_pairs, n_anchor, with_world, tag):
    """The problem form against the trajectory form on get_X of the same problem, on bytes; the _dev form."""
    cfg, desc, inp, p = clr.make_problem(ctx, cname, system, T, B)
    chain = clr.chain_of(cname)
    rng = np.random.default_rng(B + T)
    _, pl, obs = clr.world_of(chain, B, tps, rng, n_sph=n_sph)
    sph, pairs = robot_of(chain, n_sph, n_pairs, n_anchor, rng)
    if not with_world:
        pl, obs = [], None
    rb = capi.clr_robot(sph, pl, self_pairs=pairs)
    try:
        p.solve_recursive(2, True, False)
        a = p.clearance(rb, obs, tps, MARGIN, stats_group=tps)
        b = ctx.clearance_trajectories(desc, p.X(), rb, obs, tps, MARGIN, stats_group=tps)
        clr.same_outputs(a, b, f"{tag}: problem form against trajectory form")
        clr.same_outputs(clr.problem_dev(p, arrays, rb, obs if obs is not None else np.zeros((B // tps, 0, 4)), tps, MARGIN, tps), a, f"{tag}: _dev form")
        assert np.all(np.isfinite(a.clr_min)), f"{tag}: the plans are finite"
        without = p.clearance(capi.clr_robot(sph, pl), obs, tps, MARGIN) if with_world else None
        assert without is None or np.any(without.clr_min != a.clr_min), f"{tag}: the self pairs change no minimum"
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (b) terms

def build(ctx, name):
    """(cfg, desc, inp, chain, spheres, planes, obs or None, traj_per_set, pairs, weight) of a terms case."""
    cname, system, B, T, n_sph, n_obs, n_pl, tps, n_pairs, n_anchor, inner, w = CASES[name]
    rng = np.random.default_rng(4000 + sum(map(ord, name)))
    cfg, desc, inp, chain = ob.make_problem(ctx, cname, system, T, B, zero_task=(name == "one"))
    tps = B if tps is None else tps
    if inner:   # the anchor behind the second joint, the second members behind the fourth and the fifth: joints 0, 1 and 5, 6 move no pair
        seg = [s for s, j in enumerate(chain["seg_joint"]) if int(j) >= 0]
        links = [-1, seg[1], seg[3], seg[4], len(chain["seg_joint"]) - 1]
        sph = [(l, rng.uniform(-0.1, 0.1, 3), 0.0 if i == 2 else float(rng.uniform(0.02, 0.1))) for i, l in enumerate(links)]
        pairs = [(1, 3), (1, 2)]
    else:
        sph, pairs = robot_of(chain, n_sph, n_pairs, n_anchor, rng)
    obs = clr.obstacles_of(B // tps, n_obs, rng) if n_obs else None
    return cfg, desc, inp, chain, sph, ob.planes_of(n_pl), obs, tps, pairs, w


def check_terms(ctx, arrays, name):
    """Returns the worst |got - ref| / tolerance over cost, lx and lxx."""
    cfg, desc, inp, chain, sph, pl, obs, tps, pairs, w = build(ctx, name)
    dof = chain["dof"]
    margin = CASE_MARGIN.get(name, MARGIN)
    p = workloads.load_batch(ctx, desc, inp, len(inp["q0"]))
    try:
        p.set_obstacles(sph, pl, obs, margin, w, tps, self_pairs=pairs)
        p.solve_recursive(0, True, False)
        Q = p.X()[..., :dof]
        if ("terms", name) not in _REF:
            _REF["terms", name] = (Q.copy(), ref.terms(chain, Q, sph, pl, obs, pairs, tps, margin, w))
        assert _REF["terms", name][0].tobytes() == Q.tobytes(), f"{name}: the plan differs from the one the reference was computed for"
        r = _REF["terms", name][1]
        assert r["self_active"] > 0, f"{name}: no self pair is active: the case shows nothing"
        got = p.obstacle_terms()
        worst = 0.0
        for f in ("cost", "lx", "lxx"):
            g, e = getattr(got, f), r[f]
            ratio = float(np.max(np.abs(g - e) / (TOL * max(1.0, w) * np.maximum(1.0, np.abs(e)))))
            print(f"{name}: {f}: worst |error| / tolerance {ratio:.3e} ({r['self_active']} active self pairs, kink gap {float(r['kink']):.3e}, centre gap {float(r['dist']):.3e})", flush=True)
            worst = max(worst, ratio)
        assert worst <= 1.0, f"{name}: the terms are {worst:.3e} tolerances from the 50-digit reference"
        assert got.lxx.tobytes() == np.swapaxes(got.lxx, 2, 3).tobytes(), f"{name}: lxx is not exactly symmetric"
        assert np.all(got.lx[r["lx"] == 0] == 0) and np.all(got.lxx[r["lxx"] == 0] == 0), f"{name}: an entry the reference has at 0 is not 0"
        if obs is None and not pl:   # self pairs alone: the joints before the first anchor's link and behind the last second member's move no pair
            first = joints_upto(chain, min(sph[a][0] for a, _ in pairs))
            last = joints_upto(chain, max(sph[b][0] for _, b in pairs))
            out = [m for m in range(dof) if m < first or m >= last]
            if name == "inner":
                assert out == [0, 1, 5, 6], f"{name}: joints {out} move no pair"
            assert np.all(got.lx[..., out] == 0.0) and np.all(got.lxx[..., out, :] == 0.0) and np.all(got.lxx[..., :, out] == 0.0), f"{name}: joints {out} move no pair"
            assert np.any(got.lx[..., first:last] != 0.0)
        dev = ob.terms_dev(p, arrays)
        for f in ("cost", "lx", "lxx"):
            assert getattr(dev, f).tobytes() == getattr(got, f).tobytes(), f"{name}: {f} of the _dev form differs"
        return worst
    finally:
        p.close()


def check_reference_gradient(ctx):
    """The reference on itself: l_x is half the central difference of the cost, at 50 digits, on states of the smallest mapped case."""
    cfg, desc, inp, chain, sph, pl, obs, tps, pairs, w = build(ctx, "gen4")
    rng = np.random.default_rng(3)
    for t in range(2):
        ref.check_gradient(chain, rng.uniform(-2.0, 2.0, chain["dof"]), sph, pl, obs[t], pairs, MARGIN, w)


# ------------------------------------------------------------------------------------------------ (c) inert

def far_world(chain, inp, B, seed):
    """iter_world of tests/obstacles.py (an obstacle near every instance's tool: terms that act), its first sphere moved 5 m below the base, and
    three pairs on that sphere: no self pair ever comes within the margin."""
    _, pl, obs = ob.iter_world(chain, inp, seed)
    sph, pairs = robot_of(chain, 5, 3, 1, np.random.default_rng(seed))
    assert sph[0][0] == -1 and all(a == 0 for a, _ in pairs)
    return [(-1, (0.0, 0.0, -5.0), 0.01)] + sph[1:], pl, obs, pairs


def check_inert(ctx, cname, system, T, B, tag, nit=3):
    cfg, desc, inp, chain = ob.make_problem(ctx, cname, system, T, B)
    sph, pl, obs, pairs = far_world(chain, inp, B, 9)
    p, q, plain = (workloads.load_batch(ctx, desc, inp, B) for _ in range(3))
    try:
        q.set_obstacles(sph, pl, obs, ob.MARGIN, 20.0, 1)
        q.solve_recursive(nit, True, False)
        want = ob.full_results(q, cfg, nit)
        assert np.any(q.obstacle_terms(want=("cost",)).cost > 0), f"{tag}: no obstacle pair is active"
        # n_self = 0 through the keyword: the bytes of the call without it
        p.set_obstacles(sph, pl, obs, ob.MARGIN, 20.0, 1, self_pairs=[])
        p.solve_recursive(nit, True, False)
        ms.same(want, ob.full_results(p, cfg, nit), f"{tag}: self_pairs = []")
        a, b = p.clearance(capi.clr_robot(sph, pl, self_pairs=[]), obs, 1, ob.MARGIN), p.clearance(capi.clr_robot(sph, pl), obs, 1, ob.MARGIN)
        clr.same_outputs(a, b, f"{tag}: clearance with self_pairs = []")
        # pairs that stay beyond the margin
        p.set_obstacles(sph, pl, obs, ob.MARGIN, 20.0, 1, self_pairs=pairs)
        p.solve_recursive(nit, True, False)
        got = ob.full_results(p, cfg, nit)
        for k, v in want.items():
            assert np.array_equal(v, got[k], equal_nan=True), f"{tag}: pairs beyond the margin: {k} moved ({int(np.sum(v != got[k]))} entries)"
        tp, tq = p.obstacle_terms(), q.obstacle_terms()
        for f in ("cost", "lx", "lxx"):
            assert getattr(tp, f).tobytes() == getattr(tq, f).tobytes(), f"{tag}: pairs beyond the margin: {f} of the terms moved"
        # self pairs alone, beyond the margin, against a problem that never had terms; then clear_obstacles()
        plain.solve_recursive(nit, True, False)
        never = ob.full_results(plain, cfg, nit)
        p.set_obstacles(sph, [], None, ob.MARGIN, 20.0, 1, self_pairs=pairs)
        p.solve_recursive(nit, True, False)
        assert np.all(p.obstacle_terms(want=("cost",)).cost == 0)
        p.clear_obstacles()
        cl._refused(lambda: p.obstacle_terms(), "the problem has no obstacle terms")
        p.solve_recursive(nit, True, False)
        ms.same(never, ob.full_results(p, cfg, nit), f"{tag}: after clear_obstacles")
    finally:
        for h in (p, q, plain):
            h.close()


# ------------------------------------------------------------------------------------------------ (d) iterations against the restatement

#           (chain, system, T, B, al, iterations, with obstacles and planes)
ITER_CASES = (("panda", "po1", 9, 3, False, 1, True), ("panda", "po1", 9, 3, False, 3, False), ("gen4", "pot2", 5, 2, False, 1, True),
              ("panda", "po1", 9, 2, True, 1, False), ("panda", "po1", 9, 2, True, 3, True))
COOP_ITER_CASES = tuple((c, s, 9, 3, al, nit, w) for c, s in (("panda", "po1"), ("panda", "js1")) for al, nit, w in ((False, 1, True), (False, 3, False), (True, 1, False), (True, 3, True)))
W_ITER = 20.0


def iter_world(chain, inp, seed, with_world):
    """Five spheres and three pairs on two anchors (link -1 among them), with the world of obstacles.iter_world or none."""
    _, pl, obs = ob.iter_world(chain, inp, seed)
    sph, pairs = robot_of(chain, 5, 3, 2, np.random.default_rng(seed))
    if not with_world:
        pl, obs = [], None
    return sph, pl, obs, pairs


def check_iterations(ctx, cname, system, T, B, al, nit, with_world, tag, weight=W_ITER):
    """Returns the worst ratio to the tolerance of K, d and cost."""
    cfg, desc, inp, chain = ob.make_problem(ctx, cname, system, T, B, R=ob.R_C, u_scale=0.2)
    dof = chain["dof"]
    sph, pl, obs, pairs = iter_world(chain, inp, 31 + T, with_world)
    systems = ob.oracle_systems(cfg, inp, cname, B)
    p = workloads.load_batch(ctx, desc, inp, B)
    try:
        p.set_obstacles(sph, pl, obs, MARGIN, weight, 1, self_pairs=pairs)
        alr = None
        if al:
            A, b, lam = oc.set_al_rows(p, B, T, [ob.AL_ROW["row"]])
            p.solve_al(nit, nit + 1, ob.AL_ROW["penalty"], 1.1, True, False)   # lag_update_step > nb_iter: the multipliers stay
        else:
            p.solve_recursive(nit, True, False)
        K, d, cost, alpha, iters, U = p.K(), p.d(), p.cost(), p.alpha(), p.iters(), p.U()
        trace_alpha = p.trace(nit)[1]
        Q = p.X()[..., :dof]
        worst = dict(K=0.0, d=0.0, cost=0.0)
        for i in range(B):
            oi = obs[i] if obs is not None else np.zeros((0, 4))
            assert ref.state_terms(chain, Q[i, T // 2], sph, pl, oi, pairs, MARGIN, weight, derivs=False)["self_active"] > 0, f"{tag}: instance {i}: no self pair is active at the plan"
            world = ref.World(chain, sph, pl, oi, pairs, MARGIN, weight)
            if al:
                alr = dict(A=A, b=b, lam=lam[i], penalty=ob.AL_ROW["penalty"])
            r = oref.solve(systems[i], np.array([desc.R_diag[j] for j in range(p.dims.n_u)]), world, ob.x0_of(cfg, inp, i, dof), inp["U0"][i], nit, al=alr)
            assert iters[i] == nit and list(trace_alpha[i]) == r["alphas"] and alpha[i] == r["alpha"], \
                f"{tag}: instance {i}: step sizes {list(trace_alpha[i])} against the restatement's {r['alphas']}"
            eK = np.abs(K[i] - r["K"]) / (K_TOL["atol"] + K_TOL["rtol"] * np.abs(r["K"]))
            ed = np.abs(d[i] - r["d"]) / (D_TOL["atol"] + D_TOL["rtol"] * np.abs(r["d"]))
            ec = abs(cost[i] - r["cost"]) / (1e-9 * abs(r["cost"]))
            worst = dict(K=max(worst["K"], float(eK.max())), d=max(worst["d"], float(ed.max())), cost=max(worst["cost"], float(ec)))
            assert eK.max() <= 1 and ed.max() <= 1 and ec <= 1, f"{tag}: instance {i}: K {eK.max():.3e}, d {ed.max():.3e}, cost {ec:.3e} of their tolerances"
            assert np.allclose(U[i], r["U"], rtol=1e-6, atol=1e-9), f"{tag}: instance {i}: the plans differ"
        print(f"{tag}: worst / tolerance: K {worst['K']:.3e}, d {worst['d']:.3e}, cost {worst['cost']:.3e}", flush=True)
        return worst
    finally:
        p.close()


#        T, B, traj_per_set (None: B), spheres, pairs, anchors, with obstacles and planes, AL state rows: shapes of tests/test_gpu_obstacles_coop.py
SWEEP_MARGIN = 1.0   # reaches across the arm: the lone (base, tool) pair of the first shape is active at every state
SWEEP = [(2, 1, 1, 5, 1, 1, False, None), (3, 5, 5, 5, 7, 3, True, None), (9, 70, 1, 32, 64, 8, True, None), (17, 70, 5, 5, 7, 3, False, [5]),
         (33, 5, None, 5, 7, 3, True, [1, 3, 5, 6]), (9, 70, None, 5, 1, 1, False, [1, 3, 5, 6])]


def check_sweep(ctx, T, B, tps, n_sph, n_pairs, n_anchor, with_world, al_rows, tag, cname="panda", system="po1", weight=200.0):
    """One iteration in cooperative mode against generic mode (K_TOL / D_TOL), and K against the solve with the same world but without the self
    pairs (> 100 tolerances): obstacles_coop.check_sweep with self pairs."""
    cfg, desc, inp, chain = ob.make_problem(ctx, cname, system, T, B, R=ob.R_C, u_scale=0.2)
    tps = B if tps is None else tps
    _, pl, obs = oc.sweep_world(chain, inp, B, tps, n_sph, 9, 2, 100 + T + B)
    sph, pairs = robot_of(chain, n_sph, n_pairs, n_anchor, np.random.default_rng(100 + T + B))
    if not with_world:
        pl, obs = [], None
    p = workloads.load_batch(ctx, desc, inp, B)

    def solve():
        if al_rows:
            p.solve_al(1, 2, ob.AL_ROW["penalty"], 1.1, True, False)
        else:
            p.solve_recursive(1, True, False)
        return p.K(), p.d()
    try:
        if al_rows:
            oc.set_al_rows(p, B, T, al_rows)
        p.set_obstacles(sph, pl, obs, SWEEP_MARGIN, weight, tps, self_pairs=pairs)
        oc.coop(ctx, True)
        K, d = solve()
        oc.coop(ctx, False)
        p.set_controls(inp["U0"])
        Kg, dg = solve()
        eK = np.abs(K - Kg) / (K_TOL["atol"] + K_TOL["rtol"] * np.abs(Kg))
        ed = np.abs(d - dg) / (D_TOL["atol"] + D_TOL["rtol"] * np.abs(dg))
        if with_world:
            p.set_obstacles(sph, pl, obs, SWEEP_MARGIN, weight, tps)
        else:
            p.clear_obstacles()
        p.set_controls(inp["U0"])
        K0, _ = solve()
        moved = np.abs(Kg - K0) / (K_TOL["atol"] + K_TOL["rtol"] * np.abs(K0))
        print(f"{tag}: K {eK.max():.3e}, d {ed.max():.3e} of their tolerances against generic mode; the self pairs move K by {moved.max():.3e} tolerances", flush=True)
        assert np.all(np.isfinite(K)) and np.all(np.isfinite(d))
        assert eK.max() <= 1 and ed.max() <= 1, f"{tag}: K {eK.max():.3e}, d {ed.max():.3e} of their tolerances against generic mode"
        assert moved.max() > 100, f"{tag}: the self pairs move K by {moved.max():.3e} tolerances only: dropped pairs would not be seen"
        return dict(K=float(eK.max()), d=float(ed.max()))
    finally:
        oc.coop(ctx, True)
        p.close()


# ------------------------------------------------------------------------------------------------ (e) the term bites

def bite_scenario(ctx):
    """The scenario of obstacles.bite_scenario with its obstacle as a sphere of the robot's own base: one PosOrn-1 instance on the workloads'
    Panda whose cheapest plan carries the tool's sphere through a sphere on link -1.  Returns (scenario, spheres, pairs)."""
    sc = ob.bite_scenario(ctx)
    cfg, desc, inp, chain, s, x0, tool_sph, obs, free = sc
    sph = [(-1, tuple(float(v) for v in obs[0, 0, :3]), float(obs[0, 0, 3])), tool_sph[0]]
    return sc, sph, [(0, 1)]


def self_clr_min(chain, X, sph, pairs):
    return float(ref.clearance(chain, np.asarray(X)[None, :, :7], sph, [], None, pairs, 1, ob.BITE["margin"], ties=True)["clr_min"][0])


def check_bites_reference(ctx):
    """On the references alone: self-colliding without the term, clear by margin / 2 with it."""
    sc, sph, pairs = bite_scenario(ctx)
    cfg, desc, inp, chain, s, x0, _, _, free = sc
    blocked = self_clr_min(chain, free["X"], sph, pairs)
    world = ref.World(chain, sph, [], np.zeros((0, 4)), pairs, ob.BITE["margin"], ob.BITE["weight"])
    avoid = oref.solve(s, workloads.control_weights(cfg, 7), world, x0, inp["U0"][0], ob.BITE["nit"])
    cleared = self_clr_min(chain, avoid["X"], sph, pairs)
    print(f"bites: restated self clr_min {blocked:.4f} without the term, {cleared:.4f} with it (margin {ob.BITE['margin']})", flush=True)
    assert blocked < 0, f"the scenario's cheapest plan does not collide with the robot itself (clr_min {blocked})"
    assert cleared >= ob.BITE["margin"] / 2, f"the restated solve with the term ends with clr_min {cleared} (< margin / 2)"
    return sc, sph, pairs, avoid


def check_bites(ctx):
    sc, sph, pairs, avoid = check_bites_reference(ctx)
    cfg, desc, inp, chain, s, x0, _, _, free = sc
    rb = capi.clr_robot(sph, self_pairs=pairs)
    nit, margin = ob.BITE["nit"], ob.BITE["margin"]
    p = workloads.load_batch(ctx, desc, inp, 1)
    try:
        p.solve_recursive(nit, True, False)
        K_free = p.K()
        first = p.clearance(rb, None, 1, margin)
        assert first.clr_min[0] < 0 and tuple(first.clr_at[0][1:]) == (1, 0) and first.eligible[0] == 0, f"the library's plan without the term is not in self-collision: {first.clr_min}"
        p.set_obstacles(sph, [], None, margin, ob.BITE["weight"], 1, self_pairs=pairs)
        p.solve_recursive(nit, True, False)
        got = p.clearance(rb, None, 1, margin)
        assert np.allclose(p.X()[0], avoid["X"], rtol=1e-6, atol=1e-8), "the library's plan with the term is not the restated one"
        assert list(p.trace(nit)[1][0]) == avoid["alphas"], "step sizes against the restatement"
        assert got.clr_min[0] >= margin / 2, f"the library's plan with the term has self clr_min {got.clr_min[0]}"
        moved = np.abs(p.K() - K_free) / (K_TOL["atol"] + K_TOL["rtol"] * np.abs(K_free))
        assert moved.max() > 100, f"K moves by {moved.max():.3e} tolerances with the term: the check would not see it dropped"
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (f) multi-start

def check_selection(ctx, arrays, tag="selection"):
    """Five groups of three hand-written starts (clearance.check_selection's): a millimetre sphere on link -1 stands at the last position of the
    tool's sphere of every member meant to collide, paired with that sphere."""
    G, S, T = 5, 3, 9
    B = G * S
    cfg, desc, inp, p = clr.make_problem(ctx, "panda", "po1", T, B, random_controls=False)
    chain = clr.chain_of("panda")
    tool = len(chain["seg_joint"]) - 1
    for b in range(B):   # member s of group g turns joint s + 1 at its own rate
        inp["U0"][b, :, (b % S) + 1] = 0.2 + 0.05 * (b // S) + 0.1 * (b % S)
        inp["U0"][b, :, 0] = -0.1 * (1 + b % S)
    try:
        p.set_controls(inp["U0"])
        p.solve_recursive(0, True, False)
        X, cost, status = p.X(), p.cost(), p.status()
        order = [sorted(range(g * S, (g + 1) * S), key=lambda b: cost[b]) for g in range(G)]
        blocked = {0: [], 1: order[1][:1], 2: order[2][:2], 3: order[3], 4: [4 * S]}   # group 3 has no clear member
        members = [b for g in range(G) for b in blocked[g]]
        sph = []
        for b in members:
            R_, p_ = cref.link_frames(chain, X[b, T - 1, :7], tool)[tool + 1]
            c = p_ + R_ * cref.mp.matrix([0.0, 0.0, 0.05])
            sph.append((-1, (float(c[0]), float(c[1]), float(c[2])), 0.001))
        sph.append((tool, (0.0, 0.0, 0.05), 0.002))
        pairs = [(a, len(members)) for a in range(len(members))]
        assert len(members) == 7
        r = ref.clearance(chain, X[..., :7], sph, [], None, pairs, S, 0.0)
        expect = np.ones(B, np.int32)
        expect[members] = 0
        assert np.array_equal(r["eligible"], expect), f"{tag}: in self-collision {np.flatnonzero(r['eligible'] == 0)}, meant {np.flatnonzero(expect == 0)}"
        rb = capi.clr_robot(sph, self_pairs=pairs)
        got = p.clearance(rb, None, S, 0.0)
        clr.against_reference(got, r, tag)
        sel = p.select(S, None, got.eligible)
        ms.same_selection(sel, ms.select_ref(cost, got.eligible, status, S), tag)
        for g in range(G):
            clear = [b for b in order[g] if expect[b]]
            assert sel.winner[g] == (clear[0] if clear else g * S) and sel.n_candidates[g] == len(clear), f"{tag}: group {g}: winner {sel.winner[g]}, {sel.n_candidates[g]} candidates"
        assert sel.n_candidates[3] == 0 and sel.winner[3] == 3 * S and got.clr_min[3 * S] < 0
        dv = clr.problem_dev(p, arrays, rb, np.zeros((G, 0, 4)), S, 0.0, None)
        assert dv.eligible.tobytes() == got.eligible.tobytes(), f"{tag}: eligible of the _dev form"
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (g) gains

def check_gains(ctx, cname, system, T, B, al, tag):
    """The byte rules of obstacles.check_gains about a plan with active self pairs (and no other term)."""
    cfg, desc, inp, chain = ob.make_problem(ctx, cname, system, T, B, R=ob.R_C)
    sph, pl, obs, pairs = iter_world(chain, inp, 77, False)
    p, q = workloads.load_batch(ctx, desc, inp, B), workloads.load_batch(ctx, desc, inp, B)
    pen = ob.AL_ROW["penalty"]
    try:
        for h in (p, q):
            h.set_obstacles(sph, pl, obs, 1.0, 20.0, 1, self_pairs=pairs)   # a margin that reaches across every chain
            if al:
                oc.set_al_rows(h, B, T, [ob.AL_ROW["row"]])
        if al:
            p.solve_al(0, 2, pen, 1.0, True, False)
            p.gains_al(pen)
            q.solve_al(1, 2, pen, 1.0, True, False)
        else:
            p.solve_recursive(0, True, False)
            p.gains()
            q.solve_recursive(1, True, False)
        assert np.any(p.obstacle_terms(want=("cost",)).cost > 0), f"{tag}: no self pair is active at the plan"
        assert p.K().tobytes() == q.K().tobytes(), f"{tag}: K about the plan differs from the fresh one-iteration solve's"
        assert (q.alpha()[:, None, None] * p.d()).tobytes() == q.d().tobytes(), f"{tag}: d of the solve is not alpha times d about the plan"
        q.clear_obstacles()   # and the terms are in that K: without them it differs
        q.set_controls(inp["U0"])
        (q.solve_al(1, 2, pen, 1.0, True, False) if al else q.solve_recursive(1, True, False))
        assert p.K().tobytes() != q.K().tobytes(), f"{tag}: the gains do not feel the self pairs"
    finally:
        p.close()
        q.close()


# ------------------------------------------------------------------------------------------------ (h) refusals

def check_refusals(ctx, arrays, tag="refusals"):
    cfg, desc, inp, chain, sph, pl, obs, tps, pairs, w = build(ctx, "gen4")
    B = len(inp["q0"])
    p = workloads.load_batch(ctx, desc, inp, B)
    L = ctx.L
    n_sph = len(sph)

    def call(rb, n_obs=None, fn="ilqr_problem_set_obstacles"):
        world = capi.ClrWorld(obs.ctypes.data, obs.shape[0], obs.shape[1] if n_obs is None else n_obs, tps, MARGIN, 0)
        ctx.check(getattr(L, fn)(p.h, C.byref(rb), C.byref(world), 1.0))

    def robot(prs, n_self=None, spheres=sph):
        rb = capi.clr_robot(spheres, pl, self_pairs=prs)
        if n_self is not None:
            rb.n_self = n_self
        return rb

    R = cl._refused
    try:
        call(robot(pairs))   # the base call is accepted
        R(lambda: call(robot(pairs, n_self=-1)), "n_self must be 0 .. 64 (got -1)")
        R(lambda: call(robot(pairs, n_self=65)), "n_self must be 0 .. 64 (got 65)")
        R(lambda: call(robot([(0, n_sph)])), f"self_pair[0] = (0, {n_sph}) names a sphere outside 0 .. {n_sph - 1}")
        R(lambda: call(robot([pairs[0], (-1, 2)])), f"self_pair[1] = (-1, 2) names a sphere outside 0 .. {n_sph - 1}")
        R(lambda: call(robot([(2, 1)])), "self_pair[0] = (2, 1) must have a < b")
        R(lambda: call(robot([(1, 1)])), "self_pair[0] = (1, 1) must have a < b")
        R(lambda: call(robot(pairs + pairs[:1])), f"self_pair[{len(pairs)}] = ({pairs[0][0]}, {pairs[0][1]}) repeats self_pair[0]")
        # two spheres on one link; two links with a fixed segment alone between them
        two = [(-1, (0.0, 0.0, 0.0), 0.05), (-1, (0.0, 0.0, 0.3), 0.05), (len(chain["seg_joint"]) - 1, (0.0, 0.0, 0.0), 0.05)]
        R(lambda: call(robot([(0, 1)], spheres=two)), "self_pair[0] = (0, 1): both spheres are on link -1, their distance is constant")
        fixed = [s for s in range(len(chain["seg_joint"])) if int(chain["seg_joint"][s]) < 0]
        assert fixed, "the chain has no fixed segment"
        f = fixed[0]
        rigid = [(f - 1, (0.0, 0.0, 0.0), 0.05), (f, (0.0, 0.0, 0.0), 0.05)]
        R(lambda: call(robot([(0, 1)], spheres=rigid)), f"self_pair[0] = (0, 1): no moving joint lies between link {f - 1} and link {f}, their distance is constant")
        # nine anchors
        n_seg = len(chain["seg_joint"])
        many = [(-1, (0.01 * i, 0.0, 0.0), 0.01) for i in range(9)] + [(n_seg - 1, (0.0, 0.0, 0.0), 0.01)]
        R(lambda: call(robot([(i, 9) for i in range(9)], spheres=many)), "the self pairs have 9 distinct first members (anchors); at most 8 are supported")
        call(robot([(i, 9) for i in range(8)], spheres=many))
        # the bound on n_obs drops by ILQR_CLR_MAX_SPH (the check comes before anything is read through obs)
        top = (1 << 26) - 8
        R(lambda: call(robot(pairs), n_obs=top - 31), f"n_obs must be at most {top - 32} with self pairs (got {top - 31})")
        R(lambda: call(robot(pairs, n_self=-1), fn="ilqr_problem_set_obstacles_dev"), "ilqr_problem_set_obstacles_dev: n_self must be 0 .. 64")
        # the clearance calls refuse the same; with self pairs a call without obstacles and planes is legal
        p.set_obstacles(sph, pl, obs, MARGIN, w, tps, self_pairs=pairs)
        p.solve_recursive(0, True, False)
        R(lambda: p.clearance(robot([(2, 1)]), obs, tps, MARGIN), "ilqr_problem_clearance: self_pair[0] = (2, 1) must have a < b")
        R(lambda: p.clearance(capi.clr_robot(sph), None, tps, MARGIN), "nothing to keep clear of: n_obs = 0 and n_planes = 0")
        assert np.all(np.isfinite(p.clearance(capi.clr_robot(sph, self_pairs=pairs), None, tps, MARGIN).clr_min))
        # the batch solvers keep refusing a problem with terms
        psi = workloads.psi_of(dict(kind="unitstep", K=2), p.T, p.dims.n_u)
        R(lambda: p.solve_batch_cp(psi, 1, False), "obstacle terms are not supported by the batch solvers")
    finally:
        p.close()
