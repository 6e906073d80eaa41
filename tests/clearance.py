"""Clearance of plans and executions (ilqr_problem_clearance, ilqr_clearance_trajectories) -- cases and checks shared by
tests/tools/hostsim/clearance_checks.py (the host build) and tests/test_gpu_clearance.py (the device kernels).

Cases (CASES): the Panda with a tool frame, gen7 and gen4 (four joints: the problem form goes through the index map); PosOrn-1 (n_x = 7) and
PosOrnTime-2 (n_x = 15 on seven joints), so that picking q out of x is exercised; T = 2, 3, 9, 67; n = 1, 13, 70, 257 (a wave and a 256-lane block
are crossed); 1, 5 and 32 spheres with link -1, a fixed segment, the tool segment and a radius 0; 1, 3 and 9 obstacles with an unused slot; 0 and
2 planes; traj_per_set 1, 5 and n.  The 50-digit reference costs milliseconds per state, so the large n go with the small T and the few spheres.

(a) reference   clr and clr_min within TOL = 1e-12 of tests/clearance_reference.py (assert_pose's tolerance for positions of this size), clr_at,
                n_below and eligible exactly; the reference asserts the runner-up and margin gaps of its own seeds.  Host and _dev form.
(b) ties        identical states at every step, two identical spheres, two identical obstacles: step 0, the lower sphere, the lower obstacle.
(c) boundary    a clearance of exactly 0.125 against margin 0.125 and nextafter(0.125, 1).
(d) bad steps   a NaN and an inf planted: NaN, (k0, -1, -1), eligible 0, n_bad 1; every other trajectory unchanged on bytes.
(e) forms       the problem form and the trajectory form on get_X of the same problem agree on bytes in every output (0 iterations; 3 with
                early stop; on the device a split plan at B = 2048); executions of closed_loop_noise against the reference; stats on bytes against a
                restatement of its summation.
(f) selection   select with the call's `eligible` picks the cheapest clear member of every group; a group without one gives g S and 0.
(g) untouched   X, U, K, d, cost, lambda, status and the plan / gains flags are as before the call.
(h) refusals    each by its text.
Every _dev form takes its arrays through an `arrays` object, as tests/multistart.py does."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ilqr_planner_amd import capi, workloads
from tests import clearance_reference as ref
from tests import closed_loop as cl
from tests import multistart as ms
from tests.helpers import general_chain, chain_pair, urdf_text, TOOL_FRAMES

TOL = 1e-12
MARGIN = 0.05
SYSTEMS = {"po1": (capi.SYS_POS_ORN, 1), "pot2": (capi.SYS_POS_ORN_TIME, 2)}
#        name: (chain, system, n, T, spheres, obstacles, planes, traj_per_set or None for n)
CASES = {
    "one": ("panda", "po1", 1, 2, 1, 1, 0, 1),
    "gen4": ("gen4", "pot2", 13, 3, 5, 3, 2, 1),
    "gen7": ("gen7", "po1", 70, 9, 5, 3, 0, 5),
    "wide": ("panda", "pot2", 257, 2, 1, 9, 2, None),
    "long": ("panda", "po1", 1, 67, 32, 3, 2, 1),
}
#       (chain, system, T, B, traj_per_set) of the problems whose two forms are compared: gen4 goes through the index map
FORMS = (("panda", "po1", 9, 13, 1), ("gen4", "pot2", 3, 70, 5), ("gen7", "pot2", 2, 257, 257), ("gen4", "po1", 67, 5, 5))
_CHAINS = {}


def chain_of(name):
    """The library's chain dict: the Panda with the rotated tool frame of tests/helpers.py, or one of its general chains."""
    if name not in _CHAINS:
        if name == "panda0":      # the workloads' own Panda, without a tool frame
            _CHAINS[name] = workloads.panda_chain()
        elif name == "panda":
            _CHAINS[name] = chain_pair(urdf_text(), "panda_link0", "panda_tip", *TOOL_FRAMES["rotated"])[0]
        else:
            _CHAINS[name] = general_chain(name, "rotated")[0]
    return _CHAINS[name]


def desc_of(chain, system, T):
    """A descriptor for ilqr_clearance_trajectories: kind, nb_deriv, dof and the chain are all it reads."""
    kind, nd = SYSTEMS[system]
    return capi.make_desc(kind=kind, nb_deriv=nd, horizon=max(T, 2), dt=0.05, R_diag=[1e-5] * 8, chain=chain, kp_timesteps=[], kp_Q=[])


def n_x_of(chain, system):
    kind, nd = SYSTEMS[system]
    return nd * chain["dof"] + (1 if kind == capi.SYS_POS_ORN_TIME else 0)


def spheres_of(chain, n_sph, rng):
    """n_sph spheres in chain order.  With 5 or more: one on link -1, one on a fixed segment (where the chain has one), one on the tool segment, one
    of radius 0.  A single sphere sits on the tool segment."""
    n_seg = len(chain["seg_joint"])
    fixed = [s for s in range(n_seg - 1) if chain["seg_joint"][s] < 0]
    if n_sph == 1:
        links = [n_seg - 1]
    else:
        links = [-1] + fixed[:1] + [n_seg - 1] + list(rng.integers(0, n_seg, n_sph - 2 - len(fixed[:1])))
    links = sorted(int(l) for l in links)
    sph = [(l, rng.uniform(-0.1, 0.1, 3), float(rng.uniform(0.02, 0.1))) for l in links]
    if n_sph > 1:
        sph[n_sph // 2] = (sph[n_sph // 2][0], sph[n_sph // 2][1], 0.0)
    return sph


def planes_of(n_planes):
    return [((0.0, 0.0, 1.0), -0.2), ((0.6, 0.0, 0.8), -1.0)][:n_planes]


def obstacles_of(n_sets, n_obs, rng):
    """[n_sets][n_obs][4]; with 3 or more slots, one slot of every set is unused (R = -1), another one in each set."""
    obs = np.empty((n_sets, n_obs, 4))
    obs[..., 0:2] = rng.uniform(-0.8, 0.8, (n_sets, n_obs, 2))
    obs[..., 2] = rng.uniform(0.0, 1.0, (n_sets, n_obs))
    obs[..., 3] = rng.uniform(0.05, 0.2, (n_sets, n_obs))
    if n_obs >= 3:
        for s in range(n_sets):
            obs[s, (s + 1) % n_obs, 3] = -1.0
    return obs


def states_of(n, T, chain, system, rng):
    """X[n][T][n_x]: joint positions in -2.5 .. 2.5 first, anything behind them (velocities and the time state play no part)."""
    X = rng.normal(0.0, 3.0, (n, T, n_x_of(chain, system)))
    X[..., : chain["dof"]] = rng.uniform(-2.5, 2.5, (n, T, chain["dof"]))
    return X


def build(name, seed=0):
    """(chain, desc, X, spheres, planes, obs, traj_per_set) of a case."""
    cname, system, n, T, n_sph, n_obs, n_pl, tps = CASES[name]
    rng = np.random.default_rng(1000 + seed + sum(map(ord, name)))
    chain = chain_of(cname)
    tps = n if tps is None else tps
    return chain, desc_of(chain, system, T), states_of(n, T, chain, system, rng), spheres_of(chain, n_sph, rng), planes_of(n_pl), obstacles_of(n // tps, n_obs, rng), tps


_REF = {}


def reference(name):
    """The 50-digit outputs of a case, computed once (with stats over groups of traj_per_set)."""
    if name not in _REF:
        chain, desc, X, sph, pl, obs, tps = build(name)
        _REF[name] = ref.clearance(chain, X[..., : chain["dof"]], sph, pl, obs, tps, MARGIN, stats_group=tps)
    return _REF[name]


def same_outputs(a, b, tag, skip=()):
    for f in capi.Clearance._fields:
        x, y = getattr(a, f), getattr(b, f)
        if f in skip or x is None or y is None:
            continue
        assert x.tobytes() == y.tobytes(), f"{tag}: {f} differs ({int(np.sum(x != y))} entries, NaN counted)"


def against_reference(got, r, tag):
    for f in ("clr", "clr_min"):
        g, e = getattr(got, f), r[f]
        assert np.array_equal(np.isnan(g), np.isnan(e)) and np.array_equal(np.isinf(g), np.isinf(e)), f"{tag}: {f}: NaN / inf pattern"
        ok = np.isfinite(e)
        err = float(np.max(np.abs(g[ok] - e[ok]))) if np.any(ok) else 0.0
        print(f"{tag}: {f} max |error| {err:.3e} (runner-up gap {float(r['gap']):.3e}, margin gap {float(r['margin_gap']):.3e})", flush=True)
        assert err <= TOL, f"{tag}: {f} is {err:.3e} from the 50-digit reference (> {TOL})"
    assert np.array_equal(got.clr_at, r["clr_at"]), f"{tag}: clr_at {got.clr_at[np.any(got.clr_at != r['clr_at'], axis=1)][:4]} against the reference"
    assert np.array_equal(got.n_below, r["n_below"]), f"{tag}: n_below"
    assert np.array_equal(got.eligible, r["eligible"]), f"{tag}: eligible"
    if got.stats is not None and "stats" in r:
        ok = np.isfinite(r["stats"])
        assert np.array_equal(ok, np.isfinite(got.stats)) and np.max(np.abs(got.stats[ok] - r["stats"][ok]), initial=0.0) <= TOL, f"{tag}: stats"


def stats_restated(clr_min, group, margin):
    """{ mean, min, n_hit, n_bad } as the header states them: the sum in ascending order with one rounding per addition."""
    out = np.empty((len(clr_min) // group, capi.CLR_STATS))
    for g in range(len(out)):
        good = [float(v) for v in clr_min[g * group:(g + 1) * group] if not np.isnan(v)]
        s = 0.0
        for v in good:
            s = s + v
        out[g] = (s / len(good) if good else np.nan, min(good) if good else np.nan, sum(1 for v in good if v < margin), group - len(good))
    return out


def world_dev(arrays, obs, tps, margin, stats_group):
    h = arrays.put(obs)
    return h, capi.ClrWorld(arrays.ptr(h) if obs.size else None, obs.shape[0], obs.shape[1], int(tps), float(margin), int(stats_group or 0))


def outputs_dev(arrays, n, T, n_groups):
    hs = [arrays.empty((n, T)), arrays.empty(n), arrays.empty((n, 3), np.int32), arrays.empty(n, np.int32), arrays.empty(n, np.int32),
          arrays.empty((max(n_groups, 1), capi.CLR_STATS))]
    return hs, capi.ClrOut(*(arrays.ptr(h) for h in hs[:5]), arrays.ptr(hs[5]) if n_groups else None)


def collect(arrays, ctx, hs, n_groups):
    ctx.synchronize()
    got = [np.array(arrays.get(h)) for h in hs]
    return capi.Clearance(*got[:5], got[5][:n_groups] if n_groups else None)


def trajectories_dev(ctx, arrays, desc, X, rb, obs, tps, margin, stats_group):
    n, T = X.shape[0], X.shape[1]
    ng = n // stats_group if stats_group else 0
    hx = arrays.put(X)
    ho, w = world_dev(arrays, obs, tps, margin, stats_group)
    hs, out = outputs_dev(arrays, n, T, ng)
    ctx.clearance_trajectories_dev(desc, n, T, arrays.ptr(hx), rb, w, out)
    return collect(arrays, ctx, hs, ng)


def problem_dev(p, arrays, rb, obs, tps, margin, stats_group):
    ng = p.B // stats_group if stats_group else 0
    ho, w = world_dev(arrays, obs, tps, margin, stats_group)
    hs, out = outputs_dev(arrays, p.B, p.T, ng)
    p.clearance_dev(rb, w, out)
    return collect(arrays, p.ctx, hs, ng)


# ------------------------------------------------------------------------------------------------ (a) reference

def check_reference(ctx, arrays, name):
    chain, desc, X, sph, pl, obs, tps = build(name)
    r = reference(name)
    rb = capi.clr_robot(sph, pl)
    got = ctx.clearance_trajectories(desc, X, rb, obs, tps, MARGIN, stats_group=tps)
    against_reference(got, r, f"{name} host form")
    assert got.stats.tobytes() == stats_restated(got.clr_min, tps, MARGIN).tobytes(), f"{name}: stats against their restatement"
    dev = trajectories_dev(ctx, arrays, desc, X, rb, obs, tps, MARGIN, tps)
    same_outputs(dev, got, f"{name} _dev form against the host form")
    only = ctx.clearance_trajectories(desc, X, rb, obs, tps, MARGIN, want=("eligible",))
    assert only.clr is None and only.clr_min is None and only.eligible.tobytes() == got.eligible.tobytes()
    only = ctx.clearance_trajectories(desc, X, rb, obs, tps, MARGIN, stats_group=tps, want=())   # stats alone: clr_min comes from the workspace
    assert only.stats.tobytes() == got.stats.tobytes(), f"{name}: stats without clr_min"


# ------------------------------------------------------------------------------------------------ problems

def make_problem(ctx, cname, system, T, B, seed=5, random_controls=True):
    """(cfg, desc, inp, problem): a batch on the chain with random (or zero) controls, nothing solved yet."""
    base = {"po1": "C3", "pot2": "C4"}[system]
    cfg = dict(workloads.config(base), T=T)
    cfg.pop("al", None)
    cfg["solver"] = "recursive"
    chain = chain_of(cname)
    chain = dict(chain, lower=np.clip(chain["lower"], -np.pi, np.pi), upper=np.clip(chain["upper"], -np.pi, np.pi))   # a continuous joint has no limits to draw from
    desc, inp = workloads.make_batch(ctx, cfg, B=B, seed=seed, chain=chain)
    rng = np.random.default_rng(seed)
    if random_controls:
        inp["U0"] = rng.normal(0.0, 0.4, inp["U0"].shape)
    else:
        inp["U0"][:] = 0.0
    if system == "pot2":
        inp["U0"][:, :, -1] = np.sqrt(cfg["ctimes"][-1] / (T - 1))
    return cfg, desc, inp, workloads.load_batch(ctx, desc, inp, B)


# ------------------------------------------------------------------------------------------------ (b) ties, (c) boundary

def check_ties(ctx, arrays, tag="ties"):
    cfg, desc, inp, p = make_problem(ctx, "panda", "po1", 9, 13, random_controls=False)
    try:
        p.solve_recursive(0, True, False)
        X = p.X()
        assert all(X[:, k].tobytes() == X[:, 0].tobytes() for k in range(9)), f"{tag}: zero controls must repeat the state"
        chain = chain_of("panda")
        tool = len(chain["seg_joint"]) - 1
        sph = [(-1, (0.0, 0.0, 0.0), 0.01), (tool, (0.01, 0.02, 0.03), 0.05), (tool, (0.01, 0.02, 0.03), 0.05)]
        near = np.array([0.3, 0.1, 0.5, 0.05])
        obs = np.array([[[5.0, 5.0, 5.0, 0.1], near, near]])
        r = ref.clearance(chain, X[..., :7], sph, [], obs, 13, 0.0, ties=True)
        assert np.all(r["clr_at"] == (0, 1, 1)), f"{tag}: the case does not put its minimum on the doubled pair: {r['clr_at']}"
        for got in (p.clearance(capi.clr_robot(sph), obs), problem_dev(p, arrays, capi.clr_robot(sph), obs, 13, 0.0, None),
                    ctx.clearance_trajectories(desc, X, capi.clr_robot(sph), obs)):
            assert np.all(got.clr_at == (0, 1, 1)), f"{tag}: clr_at {got.clr_at} (step 0, the lower sphere, the lower obstacle)"
            assert np.max(np.abs(got.clr_min - r["clr_min"])) <= TOL
    finally:
        p.close()


def check_boundary(ctx, arrays, tag="boundary"):
    chain, desc, X, _, _, _, _ = build("gen4")
    n, T = X.shape[0], X.shape[1]
    rb = capi.clr_robot([(-1, (0.0, 0.0, 0.5), 0.25)], [((0.0, 0.0, 1.0), 0.125)])
    for margin, elig, below in ((0.125, 1, 0), (np.nextafter(0.125, 1.0), 0, T)):
        for got in (ctx.clearance_trajectories(desc, X, rb, None, margin=margin), trajectories_dev(ctx, arrays, desc, X, rb, np.zeros((1, 0, 4)), n, margin, None)):
            assert np.all(got.clr == 0.125) and np.all(got.clr_min == 0.125), f"{tag}: the clearance is 0.125 exactly, got {got.clr_min}"
            assert np.all(got.eligible == elig) and np.all(got.n_below == below), f"{tag}: margin {margin!r}: eligible {got.eligible}, n_below {got.n_below}"
            assert np.all(got.clr_at == (0, 0, 0)), f"{tag}: clr_at {got.clr_at}"


# ------------------------------------------------------------------------------------------------ (d) bad steps

def check_bad_steps(ctx, arrays, name="gen7", tag="bad steps"):
    chain, desc, X, sph, pl, obs, tps = build(name)
    n, T = X.shape[0], X.shape[1]
    rb = capi.clr_robot(sph, pl)
    clean = ctx.clearance_trajectories(desc, X, rb, obs, tps, MARGIN, stats_group=tps)
    Xb = X.copy()
    planted = {7: (T - 2, 0, np.nan), 8: (1, 1, np.inf), n - 1: (0, 0, -np.inf)}   # trajectory: (step, joint, value); 7 and 8 share a group of 5
    for t, (k, j, v) in planted.items():
        Xb[t, k, j] = v
    Xb[7, T - 1, 1] = np.nan                    # a second bad step later in the same trajectory: the lowest one is named
    for got in (ctx.clearance_trajectories(desc, Xb, rb, obs, tps, MARGIN, stats_group=tps), trajectories_dev(ctx, arrays, desc, Xb, rb, obs, tps, MARGIN, tps)):
        others = np.array([t not in planted for t in range(n)])
        for t, (k, j, v) in planted.items():
            assert np.isnan(got.clr_min[t]) and tuple(got.clr_at[t]) == (k, -1, -1) and got.eligible[t] == 0, f"{tag}: trajectory {t}: {got.clr_min[t]}, {got.clr_at[t]}"
            assert np.isnan(got.clr[t, k]) and got.clr[t][~np.isnan(got.clr[t])].tobytes() == clean.clr[t][~np.isnan(got.clr[t])].tobytes()
        for f in ("clr", "clr_min", "clr_at", "n_below", "eligible"):
            assert getattr(got, f)[others].tobytes() == getattr(clean, f)[others].tobytes(), f"{tag}: {f} of an untouched trajectory moved"
        n_bad = np.zeros(n // tps)
        for t in planted:
            n_bad[t // tps] += 1
        assert np.array_equal(got.stats[:, 3], n_bad), f"{tag}: n_bad {got.stats[:, 3]} against {n_bad}"
        assert got.stats.tobytes() == stats_restated(got.clr_min, tps, MARGIN).tobytes(), f"{tag}: stats against their restatement"


# ------------------------------------------------------------------------------------------------ (e) the two forms

def world_of(chain, B, tps, rng, n_sph=5, n_obs=3, n_pl=2):
    return spheres_of(chain, n_sph, rng), planes_of(n_pl), obstacles_of(B // tps, n_obs, rng)


def check_forms(ctx, arrays, cname, system, T, B, tps, tag):
    cfg, desc, inp, p = make_problem(ctx, cname, system, T, B)
    rng = np.random.default_rng(B + T)
    sph, pl, obs = world_of(chain_of(cname), B, tps, rng)
    rb = capi.clr_robot(sph, pl)
    try:
        for nit, early in ((0, False), (3, True)):
            p.solve_recursive(nit, True, early)
            X = p.X()
            a = p.clearance(rb, obs, tps, MARGIN, stats_group=tps)
            b = ctx.clearance_trajectories(desc, X, rb, obs, tps, MARGIN, stats_group=tps)
            same_outputs(a, b, f"{tag} after {nit} iterations: problem form against trajectory form")
            same_outputs(problem_dev(p, arrays, rb, obs, tps, MARGIN, tps), a, f"{tag} after {nit} iterations: _dev form")
            assert np.all(np.isfinite(a.clr_min)), f"{tag}: the plans are finite"
            assert a.stats.tobytes() == stats_restated(a.clr_min, tps, MARGIN).tobytes(), f"{tag}: stats against their restatement"
    finally:
        p.close()


def check_split_plan(ctx, arrays, tag="split plan"):
    """B = 2048 of C4 under AUTO: the plan was left by two halves on two streams (tests/multistart.SPLIT_CASES)."""
    B, T = ms.BIG[0] * ms.BIG[1], 9
    cfg, desc, inp = ms.make_case(ctx, "C4", T, B)
    p = workloads.load_batch(ctx, desc, inp, B)
    rng = np.random.default_rng(11)
    sph, pl, obs = world_of(chain_of("panda0"), B, 16, rng)
    rb = capi.clr_robot(sph, pl)
    try:
        p.solve_recursive(3, True, True)
        a = problem_dev(p, arrays, rb, obs, 16, MARGIN, 16)
        b = ctx.clearance_trajectories(desc, p.X(), rb, obs, 16, MARGIN, stats_group=16)
        same_outputs(a, b, f"{tag}: problem form against trajectory form")
    finally:
        p.close()


def check_executions(ctx, arrays, tag="executions"):
    """X of closed_loop_noise with S = 3, n = B S, traj_per_set = stats_group = S, against the reference."""
    B, S, T = 5, 3, 9
    cfg, desc, inp, p = make_problem(ctx, "gen7", "po1", T, B)
    chain = chain_of("gen7")
    rng = np.random.default_rng(77)
    sph, pl, obs = world_of(chain, B * S, S, rng)
    rb = capi.clr_robot(sph, pl)
    try:
        p.solve_recursive(2, True, False)
        X = p.closed_loop_noise(S, 99, sigma_w=0.01, sigma_x0=0.02, want_X=True).X.reshape(B * S, T, -1)
        r = ref.clearance(chain, X[..., : chain["dof"]], sph, pl, obs, S, MARGIN, stats_group=S)
        got = ctx.clearance_trajectories(desc, X, rb, obs, S, MARGIN, stats_group=S)
        against_reference(got, r, tag)
        assert got.stats.tobytes() == stats_restated(got.clr_min, S, MARGIN).tobytes(), f"{tag}: stats against their restatement"
        same_outputs(trajectories_dev(ctx, arrays, desc, X, rb, obs, S, MARGIN, S), got, f"{tag}: _dev form")
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (f) selection

def check_selection(ctx, arrays, tag="selection"):
    G, S, T = 5, 3, 9
    B = G * S
    cfg, desc, inp, p = make_problem(ctx, "panda", "po1", T, B, random_controls=False)
    chain = chain_of("panda")
    tool = len(chain["seg_joint"]) - 1
    for b in range(B):   # hand-written controls: member s of group g turns joint s + 1 at its own rate
        inp["U0"][b, :, (b % S) + 1] = 0.2 + 0.05 * (b // S) + 0.1 * (b % S)
        inp["U0"][b, :, 0] = -0.1 * (1 + b % S)
    sph = [(tool, (0.0, 0.0, 0.05), 0.002)]   # millimetres: the starts of a group lie centimetres apart
    rb = capi.clr_robot(sph)
    try:
        p.set_controls(inp["U0"])
        p.solve_recursive(0, True, False)
        X, cost, status = p.X(), p.cost(), p.status()
        order = [sorted(range(g * S, (g + 1) * S), key=lambda b: cost[b]) for g in range(G)]
        blocked = {0: [], 1: order[1][:1], 2: order[2][:2], 3: order[3], 4: [4 * S]}   # group 3 has no clear member
        obs = np.tile(np.array([9.0, 9.0, 9.0, -1.0]), (G, S, 1))                      # unused slots
        for g, members in blocked.items():
            for slot, b in enumerate(members):   # on the path of member b: the centre of its sphere at the last step, where the paths lie apart
                R_, p_ = ref.link_frames(chain, X[b, T - 1, :7], tool)[tool + 1]
                c = p_ + R_ * ref.mp.matrix([0.0, 0.0, 0.05])
                obs[g, slot] = (float(c[0]), float(c[1]), float(c[2]), 0.001)
        r = ref.clearance(chain, X[..., :7], sph, [], obs, S, 0.0)
        expect_elig = np.ones(B, np.int32)
        for members in blocked.values():
            expect_elig[members] = 0
        assert np.array_equal(r["eligible"], expect_elig), f"{tag}: the obstacles block {np.flatnonzero(r['eligible'] == 0)}, meant {np.flatnonzero(expect_elig == 0)}"
        got = p.clearance(rb, obs, S, 0.0)
        against_reference(got, r, tag)
        sel = p.select(S, None, got.eligible)
        win, best, ncand = ms.select_ref(cost, got.eligible, status, S)
        ms.same_selection(sel, (win, best, ncand), tag)
        for g in range(G):
            clear = [b for b in order[g] if expect_elig[b]]
            assert sel.winner[g] == (clear[0] if clear else g * S) and sel.n_candidates[g] == len(clear), f"{tag}: group {g}: winner {sel.winner[g]}, {sel.n_candidates[g]} candidates"
        assert sel.n_candidates[3] == 0 and sel.winner[3] == 3 * S and got.clr_min[3 * S] < 0
        # the same through device pointers: eligible goes from one call into the other without leaving the device
        dv = problem_dev(p, arrays, rb, obs, S, 0.0, None)
        he = arrays.put(dv.eligible.astype(np.int32))
        hw, hb, hn = arrays.empty(G, np.int32), arrays.empty(G), arrays.empty(G, np.int32)
        p.select_dev(S, None, arrays.ptr(he), arrays.ptr(hw), arrays.ptr(hb), arrays.ptr(hn))
        ctx.synchronize()
        assert np.array_equal(np.array(arrays.get(hw)), sel.winner) and np.array_equal(np.array(arrays.get(hn)), sel.n_candidates)
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (g) nothing else moves

def check_untouched(ctx, arrays, tag="untouched"):
    B, T = 13, 9
    cfg = dict(workloads.config("C3"), T=T)
    chain = chain_of("panda0")
    desc, inp = workloads.make_batch(ctx, cfg, B=B, seed=3)
    p = workloads.load_batch(ctx, desc, inp, B)   # C3 carries an AL row: multipliers exist
    rng = np.random.default_rng(5)
    sph, pl, obs = world_of(chain, B, 1, rng)
    rb = capi.clr_robot(sph, pl)
    al = cfg["al"]
    try:
        cl._refused(lambda: p.clearance(rb, obs, 1, MARGIN), "ilqr_problem_clearance needs a plan")
        p.solve_al(0, al["lag"], al["penalty"], al["scaling"], True, False)   # a plan, no gains
        p.clearance(rb, obs, 1, MARGIN)
        cl._refused(lambda: p.closed_loop(samples=1), "")                     # still no gains: the call did not make any
        p.solve_al(3, 2, al["penalty"], al["scaling"], True, False)
        before = ms.results(p, cfg)
        a = p.clearance(rb, obs, 1, MARGIN, stats_group=1)
        problem_dev(p, arrays, rb, obs, 1, MARGIN, 1)
        ms.same(before, ms.results(p, cfg), f"{tag}: after ilqr_problem_clearance")
        c1 = p.closed_loop(samples=1)[0]      # the gains of the solve still count
        p.gains()
        c2 = p.closed_loop(samples=1)[0]
        assert np.all(np.isfinite(c1)) and np.all(np.isfinite(c2))
        assert p.clearance(rb, obs, 1, MARGIN, stats_group=1).clr_min.tobytes() == a.clr_min.tobytes(), f"{tag}: the same plan, the same clearance"
        p.set_controls(inp["U0"])
        cl._refused(lambda: p.clearance(rb, obs, 1, MARGIN), "ilqr_problem_clearance needs a plan")
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (h) refusals

def check_refusals(ctx, arrays, tag="refusals"):
    chain, desc, X, sph, pl, obs, tps = build("gen4")
    n, T = X.shape[0], X.shape[1]
    n_seg = len(chain["seg_joint"])
    L = ctx.L

    def call(rb=None, w=None, out=None, d=desc, n_=n, T_=T, null=()):
        rb = rb if rb is not None else capi.clr_robot(sph, pl)
        w = w if w is not None else capi.ClrWorld(obs.ctypes.data, obs.shape[0], obs.shape[1], tps, MARGIN, tps)
        keep = [np.empty(n_ * max(T_, 1) * 3 + 64)]
        out = out if out is not None else capi.ClrOut(None, keep[0].ctypes.data, None, None, None, None)
        args = [C.byref(rb) if "robot" not in null else None, C.byref(w) if "world" not in null else None, C.byref(out) if "out" not in null else None]
        ctx.check(L.ilqr_clearance_trajectories(ctx.h, C.byref(d), n_, T_, X.ctypes.data, *args))

    def robot(field=None, value=None, i=None, a=None):
        """The case's robot with one entry changed: field, field[i] or field[i][a]."""
        rb = capi.clr_robot(sph, pl)
        if field is not None and i is None:
            setattr(rb, field, value)
        elif field is not None and a is None:
            getattr(rb, field)[i] = value
        elif field is not None:
            getattr(rb, field)[i][a] = value
        return rb

    def world(**kw):
        w = capi.ClrWorld(obs.ctypes.data, obs.shape[0], obs.shape[1], tps, MARGIN, tps)
        for k, v in kw.items():
            setattr(w, k, v)
        return w

    call()   # the base call is accepted
    R = cl._refused
    R(lambda: call(null=("robot",)), "robot is a null pointer")
    R(lambda: call(null=("world",)), "world is a null pointer")
    R(lambda: call(null=("out",)), "out is a null pointer")
    R(lambda: call(rb=robot("n_sph", 0)), "n_sph must be 1 .. 32 (got 0)")
    R(lambda: call(rb=robot("n_sph", 33)), "n_sph must be 1 .. 32 (got 33)")
    R(lambda: call(rb=robot("sph_link", -2, 0)), "sph_link[0] = -2 is outside -1 .. " + str(n_seg - 1))
    R(lambda: call(rb=robot("sph_link", n_seg, 4)), f"sph_link[4] = {n_seg} is outside -1 .. {n_seg - 1}")
    R(lambda: call(rb=robot("sph_link", n_seg - 1, 0)), "sph_link must be non-decreasing")
    R(lambda: call(rb=robot("sph_r", -0.01, 1)), "sph_r[1] must be finite and >= 0")
    R(lambda: call(rb=robot("sph_r", np.inf, 1)), "sph_r[1] must be finite and >= 0")
    R(lambda: call(rb=robot("sph_c", np.nan, 2, 1)), "sph_c[2][1] is not finite")
    R(lambda: call(rb=robot("n_planes", -1)), "n_planes must be 0 .. 8 (got -1)")
    R(lambda: call(rb=robot("n_planes", 9)), "n_planes must be 0 .. 8 (got 9)")
    R(lambda: call(rb=robot("plane_n", 0.6 + 1e-8, 1, 0)), "plane_n[1] is not a unit vector")
    R(lambda: call(rb=robot("plane_n", np.inf, 0, 2)), "plane_n[0] is not finite")
    R(lambda: call(rb=robot("plane_d", np.nan, 1)), "plane_d[1] is not finite")
    R(lambda: call(w=world(n_obs=-1)), "n_obs must be >= 0 (got -1)")
    R(lambda: call(rb=robot("n_planes", 0), w=world(n_obs=0)), "nothing to keep clear of: n_obs = 0 and n_planes = 0")
    R(lambda: call(w=world(obs=None)), "obs is a null pointer with n_obs = 3")
    R(lambda: call(w=world(traj_per_set=2, n_sets=6)), "is not a multiple of traj_per_set (2)")
    R(lambda: call(w=world(traj_per_set=0)), "is not a multiple of traj_per_set (0)")
    R(lambda: call(w=world(n_sets=12)), "n_sets must be n / traj_per_set = 13 (got 12)")
    R(lambda: call(w=world(margin=np.nan)), "margin is NaN")
    R(lambda: call(out=capi.ClrOut()), "every output is a null pointer")
    keep = np.empty(n * 4)
    R(lambda: call(w=world(stats_group=0), out=capi.ClrOut(None, None, None, None, None, keep.ctypes.data)), "stats needs stats_group >= 1 (got 0)")
    R(lambda: call(w=world(stats_group=2), out=capi.ClrOut(None, None, None, None, None, keep.ctypes.data)), "is not a multiple of stats_group (2)")
    call(w=world(stats_group=0))   # stats_group is read only where stats is asked for
    R(lambda: call(n_=0), "n and T must be >= 1")
    bad = obs.copy()
    bad[2, 1, 0] = np.nan
    R(lambda: call(w=capi.ClrWorld(bad.ctypes.data, obs.shape[0], obs.shape[1], tps, MARGIN, tps)), "obs[2][1][0] is not finite")
    nochain = desc_of(chain, "pot2", T)
    nochain.n_seg = 0
    R(lambda: call(d=nochain), "the descriptor has no chain (n_seg = 0)")
    wrong = desc_of(chain, "pot2", T)
    wrong.dof = 3
    R(lambda: call(d=wrong), "the descriptor's chain is refused: chain has 4 moving joints, descriptor says 3")
    # the _dev form checks the same things but cannot look into obs
    hs, out = outputs_dev(arrays, n, T, 0)
    hx = arrays.put(X)
    R(lambda: ctx.clearance_trajectories_dev(desc, n, T, arrays.ptr(hx), robot("n_sph", 0), world(), out), "ilqr_clearance_trajectories_dev: n_sph must be 1 .. 32")


# ------------------------------------------------------------------------------------------------ (i) the class level

def multistart_world(G, rng):
    """Spheres on the workloads' Panda, one set of obstacles per task in the arm's reach, and a last set that nothing clears."""
    chain = chain_of("panda0")
    sph = spheres_of(chain, 5, rng)
    obs = np.empty((G, 3, 4))
    obs[..., 0] = rng.uniform(0.2, 0.7, (G, 3))
    obs[..., 1] = rng.uniform(-0.4, 0.4, (G, 3))
    obs[..., 2] = rng.uniform(0.1, 0.8, (G, 3))
    obs[..., 3] = 0.1
    obs[:, 1, 3] = -1.0                    # an unused slot
    obs[G - 1, 0] = (0.0, 0.0, 0.0, 5.0)   # the last task stands inside an obstacle
    return sph, [((0.0, 0.0, 1.0), -0.5)], obs


def multistart_by_hand(ctx, cfg, desc, inp, S, seed, sigma, coarse_iter, nb_iter, rb, obs, margin):
    """solveMultiStart with obstacles through capi.BatchProblem: tests/multistart.multistart_by_hand with the clearance of the starts between the
    coarse solves and the selection, and the clearance of the polished plans at the end."""
    G = len(inp["q0"])
    B = G * S
    al = ms.is_al(cfg)
    tasks = workloads.load_batch(ctx, desc, inp, G)
    starts = capi.BatchProblem(ctx, desc, B)
    try:
        if al:
            starts.set_constraints(inp["A"], inp["b"], np.repeat(inp["lambda0"], S, axis=0))
        starts.adopt(tasks, np.arange(B) // S, capi.ADOPT_STATE | capi.ADOPT_TARGETS | capi.ADOPT_CONTROLS0)
        starts.spread_controls(S, seed, sigma)
        ms.solve(starts, cfg, coarse_iter)
        coarse = starts.clearance(rb, obs, S, margin, want=("clr_min", "eligible"))
        sel = starts.select(S, None, coarse.eligible)
        tasks.adopt(starts, sel.winner, capi.ADOPT_CONTROLS | (capi.ADOPT_MULTIPLIERS if al else 0))
        ms.solve(tasks, cfg, nb_iter, ms.final_penalty(coarse_iter, cfg["al"]["lag"], cfg["al"]["penalty"], cfg["al"]["scaling"]) if al else None)
        r = dict(X=tasks.X(), U=tasks.U(), cost=tasks.cost(), alpha=tasks.alpha(), iters=tasks.iters(), status=tasks.status())
        return r, sel, coarse, tasks.clearance(rb, obs, 1, margin, want=("clr_min", "clr_at", "n_below"))
    finally:
        tasks.close()
        starts.close()
