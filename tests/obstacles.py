"""Obstacle terms in the stage cost of the Riccati solvers (ilqr_problem_set_obstacles, ilqr_problem_obstacle_terms) -- cases and checks shared by
tests/tools/hostsim/obstacle_checks.py (the host build) and tests/test_gpu_obstacles.py (the device kernels).

Cases (CASES): T = 2, 3, 9; B = 1, 13, 70 (a wave is crossed); 1, 5 and 32 spheres with link -1, a fixed segment, the tool segment and a radius 0;
1 and 9 obstacles with an unused slot; 0 and 2 planes; traj_per_set 1, 5 and B; the Panda with a tool frame, gen7 and gen4 (four joints: the
padded joints must get nothing); PosOrn-1, PosOrn-2, PosOrnTime-2 and JointSpace-1 with a chain.  B <= 70 and T <= 25 throughout: problems with
these terms run on the generic kernels.

(a) terms      obstacle_terms() on a 0-iteration plan within 1e-12 max(1, w) max(1, |ref|) of the 50-digit reference (the clearance tests' 1e-12,
               scaled by the weight); lxx exactly symmetric; the _dev form on bytes; on the T = 2 case, whose keypoint and limit terms are zero,
               get_cost is the sum of the two steps' cost bits.  The worst ratio to the tolerance is returned (profiles/obstacle_parity.txt).
(b) inert      every pair beyond the margin, and separately weight 0: X, U, K, d, cost, alpha, iters and the trace == the generic-pinned solve
               of the problem without obstacles; after clear_obstacles() the unpinned solve gives the bytes of a problem that never had any.
(c) iterations one and three iterations of the recursive and the AL solve (one row, no multiplier update) against the float64 restatement of
               tests/obstacle_reference.py: K, d at K_TOL / D_TOL of tests/gains.py, cost at rtol 1e-9, step sizes and iteration counts exactly.
(d) bites      the restated solve ends with clr_min < 0 without the term and >= margin / 2 with it (shown on the reference alone); the
               library's plan, scored by ilqr_problem_clearance, is held to it; K differs from the K without obstacles by > 100 tolerances.
(e) gains      gains() / gains_al() about an obstacle plan: K of a fresh one-iteration solve from the same controls on bytes, d alpha times it.
(f) untouched  obstacle_terms leaves X, U, K, d, cost, lambda, status and the flags as they were.
(g) refusals   each by its text; the batch solvers' refusal."""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

from ilqr_planner_amd import capi, workloads
from tests import clearance as clr
from tests import clearance_reference as cref
from tests import closed_loop as cl
from tests import multistart as ms
from tests import narrow_chain as nc
from tests import obstacle_reference as ref
from tests.gains import D_TOL, K_TOL
from tests.helpers import TOOL_FRAMES, chain_pair, general_chain, oracle_system_of_instance, urdf_text

TOL = 1e-12
MARGIN = 0.15
#         name: (kind, nb_deriv, the workload whose precisions and times it borrows)
SYSTEMS = {"po1": (capi.SYS_POS_ORN, 1, "C2"), "po2": (capi.SYS_POS_ORN, 2, "C2nd"), "pot2": (capi.SYS_POS_ORN_TIME, 2, "C4"), "js1": (capi.SYS_JOINT, 1, "C1j")}
#       name: (chain, system, B, T, spheres, obstacles, planes, traj_per_set or None for B, weight)
CASES = {
    "one": ("panda", "po1", 1, 2, 1, 1, 0, 1, 50.0),
    "gen4": ("gen4", "pot2", 13, 3, 5, 9, 2, 1, 0.5),
    "gen7": ("gen7", "po2", 70, 2, 5, 1, 0, 5, 3.0),
    "shared": ("gen4", "po1", 13, 2, 5, 9, 2, None, 200.0),
    "long": ("panda", "js1", 1, 9, 32, 9, 2, None, 7.0),
}
_SEGS = {}


@contextlib.contextmanager
def generic_pin(on=True):
    """The generic kernel set for the solves inside the block (every solve of capi.BatchProblem re-applies the environment's switches)."""
    old = os.environ.get("ILQR_HIP_PATH")
    os.environ["ILQR_HIP_PATH"] = "v1" if on else "v2"
    try:
        yield
    finally:
        if old is None:
            del os.environ["ILQR_HIP_PATH"]
        else:
            os.environ["ILQR_HIP_PATH"] = old


def segs_of(name):
    """The oracle's segments of the chains of tests/clearance.chain_of."""
    if name not in _SEGS:
        if name == "panda0":
            from tests.helpers import panda_segs
            _SEGS[name] = panda_segs()
        elif name == "panda":
            _SEGS[name] = chain_pair(urdf_text(), "panda_link0", "panda_tip", *TOOL_FRAMES["rotated"])[1]
        else:
            _SEGS[name] = general_chain(name, "rotated")[1]
    return _SEGS[name]


def planes_of(n_planes):
    """The floor 10 cm above the base (a sphere on link -1 is below it: an active plane pair at every step) and a far wall."""
    return [((0.0, 0.0, 1.0), 0.1), ((0.6, 0.0, 0.8), -1.0)][:n_planes]


def with_chain(desc, chain):
    """The descriptor of a joint-space batch (which has no chain of its own) with the segments of `chain`."""
    n = len(chain["seg_joint"])
    desc.n_seg = n
    for i in range(n):
        desc.seg_joint[i] = int(chain["seg_joint"][i])
        for k in range(3):
            desc.seg_xyz[i][k] = float(chain["seg_xyz"][i][k])
            desc.seg_axis[i][k] = float(chain["seg_axis"][i][k])
        for k in range(9):
            desc.seg_R[i][k] = float(chain["seg_R"][i][k])
    return desc


def make_problem(ctx, cname, system, T, B, seed=5, zero_task=False, R=None, u_scale=0.4):
    """(cfg, desc, inp, chain): a batch of `system` on the chain with random controls, nothing loaded.  zero_task: zero precisions and zero
    controls (the stage cost without obstacles is 0 exactly).  R: one control weight for every joint."""
    kind, nd, base = SYSTEMS[system]
    cfg = dict(workloads.config(base), T=T)
    cfg.pop("al", None)
    cfg["solver"] = "recursive"
    if zero_task:
        cfg["Qdiag"] = [[0.0] * len(q) for q in cfg["Qdiag"]]
    if R is not None:
        cfg["R_diag"] = [R] * 7
    chain = clr.chain_of(cname)
    chain = dict(chain, lower=np.clip(chain["lower"], -np.pi, np.pi), upper=np.clip(chain["upper"], -np.pi, np.pi))
    if system == "js1":
        assert chain["dof"] == 7, "the joint-space workloads are built for 7 joints"
        desc, inp = workloads.make_batch(ctx, cfg, B=B, seed=seed)
        desc = with_chain(desc, chain)
    else:
        desc, inp = workloads.make_batch(ctx, cfg, B=B, seed=seed, chain=chain)
    rng = np.random.default_rng(seed)
    inp["U0"] = np.zeros_like(inp["U0"]) if zero_task else rng.normal(0.0, u_scale, inp["U0"].shape)
    if kind == capi.SYS_POS_ORN_TIME:
        inp["U0"][:, :, -1] = np.sqrt(cfg["ctimes"][-1] / (T - 1))
    return cfg, desc, inp, chain


def build(ctx, name):
    """(cfg, desc, inp, chain, spheres, planes, obs, traj_per_set, weight) of a case."""
    cname, system, B, T, n_sph, n_obs, n_pl, tps, w = CASES[name]
    rng = np.random.default_rng(2000 + sum(map(ord, name)))
    cfg, desc, inp, chain = make_problem(ctx, cname, system, T, B, zero_task=(name == "one"))
    tps = B if tps is None else tps
    sph, obs = clr.spheres_of(chain, n_sph, rng), clr.obstacles_of(B // tps, n_obs, rng)
    if n_obs == 1:   # a lone random obstacle is rarely within the margin: put it 6 cm from the tool frame of the set's first instance at q0
        for s in range(B // tps):
            near_tool(chain, inp["q0"][s * tps], obs[s, 0])
    return cfg, desc, inp, chain, sph, planes_of(n_pl), obs, tps, w


_REF = {}


def reference(name, chain, Q, sph, pl, obs, tps, w):
    """The 50-digit terms of a case's plan, computed once per process (the plan is a rollout of fixed inputs)."""
    if name not in _REF:
        _REF[name] = (Q.copy(), ref.terms(chain, Q, sph, pl, obs, tps, MARGIN, w))
    assert _REF[name][0].tobytes() == Q.tobytes(), f"{name}: the plan differs from the one the reference was computed for"
    return _REF[name][1]


# ------------------------------------------------------------------------------------------------ (a) terms against the reference

def terms_dev(p, arrays):
    dof = int(p.desc.dof)
    hs = [arrays.empty((p.B, p.T)), arrays.empty((p.B, p.T, dof)), arrays.empty((p.B, p.T, dof, dof))]
    p.obstacle_terms_dev(*(arrays.ptr(h) for h in hs))
    p.ctx.synchronize()
    return capi.ObstacleTerms(*(np.array(arrays.get(h)) for h in hs))


def check_terms(ctx, arrays, name):
    """Returns the worst |got - ref| / tolerance over cost, lx and lxx."""
    cfg, desc, inp, chain, sph, pl, obs, tps, w = build(ctx, name)
    dof = chain["dof"]
    p = workloads.load_batch(ctx, desc, inp, len(inp["q0"]))
    try:
        p.set_obstacles(sph, pl, obs, MARGIN, w, tps)
        p.solve_recursive(0, True, False)
        X = p.X()
        r = reference(name, chain, X[..., :dof], sph, pl, obs, tps, w)
        got = p.obstacle_terms()
        assert np.any(r["cost"] > 0), f"{name}: no pair is active: the case shows nothing"
        worst = 0.0
        for f in ("cost", "lx", "lxx"):
            g, e = getattr(got, f), r[f]
            ratio = float(np.max(np.abs(g - e) / (TOL * max(1.0, w) * np.maximum(1.0, np.abs(e)))))
            print(f"{name}: {f}: worst |error| / tolerance {ratio:.3e} (kink gap {float(r['kink']):.3e}, centre gap {float(r['dist']):.3e})", flush=True)
            worst = max(worst, ratio)
        assert worst <= 1.0, f"{name}: the terms are {worst:.3e} tolerances from the 50-digit reference"
        assert got.lxx.tobytes() == np.swapaxes(got.lxx, 2, 3).tobytes(), f"{name}: lxx is not exactly symmetric"
        if dof < 7 or len(sph) > 1:   # some joint moves no sphere, or some sphere is moved by few joints: zero columns exist in the reference
            assert np.all(got.lx[r["lx"] == 0] == 0) and np.all(got.lxx[r["lxx"] == 0] == 0), f"{name}: an entry the reference has at 0 is not 0"
        dev = terms_dev(p, arrays)
        for f in ("cost", "lx", "lxx"):
            assert getattr(dev, f).tobytes() == getattr(got, f).tobytes(), f"{name}: {f} of the _dev form differs"
        only = p.obstacle_terms(want=("lx",))
        assert only.cost is None and only.lxx is None and only.lx.tobytes() == got.lx.tobytes()
        if name == "one":   # zero precisions, zero controls, inactive limits: the cost is the obstacle share alone
            c = p.cost()
            assert c[0] == got.cost[0, 0] + got.cost[0, 1] and c[0] > 0, f"{name}: get_cost {c[0]!r} against the steps' {got.cost[0]!r}"
        return worst
    finally:
        p.close()


def check_reference_gradient(ctx):
    """(i) on itself: l_x is half the central difference of c_obs, at 50 digits, on states of the smallest mapped case."""
    cfg, desc, inp, chain, sph, pl, obs, tps, w = build(ctx, "gen4")
    rng = np.random.default_rng(3)
    for t in range(2):
        ref.check_gradient(chain, rng.uniform(-2.0, 2.0, chain["dof"]), sph, pl, obs[t], MARGIN, w)


# ------------------------------------------------------------------------------------------------ (b) terms that never act

FAR = np.array([[[50.0, 50.0, 50.0, 0.1], [0.0, 0.0, 0.0, -1.0]]])   # one set: an obstacle nothing reaches and an unused slot at the base


def full_results(p, cfg, nit):
    r = ms.results(p, cfg)
    r["alpha"] = p.alpha()
    r["trace_cost"], r["trace_alpha"] = p.trace(nit)
    return r


def check_inert(ctx, cname, system, T, B, tag, nit=3, unpinned=True):
    """unpinned = False (the host build, which has the generic kernels only): the solves after clear_obstacles() stay pinned."""
    cfg, desc, inp, chain = make_problem(ctx, cname, system, T, B)
    sph = clr.spheres_of(chain, 5, np.random.default_rng(9))
    near = clr.obstacles_of(1, 3, np.random.default_rng(10))
    p, q = workloads.load_batch(ctx, desc, inp, B), workloads.load_batch(ctx, desc, inp, B)
    try:
        with generic_pin():
            q.solve_recursive(nit, True, False)
            plain = full_results(q, cfg, nit)
            for what, obs, w in (("every pair beyond the margin", FAR, 10.0), ("weight 0", near, 0.0)):
                p.set_obstacles(sph, [], obs, MARGIN, w)
                p.solve_recursive(nit, True, False)
                got = full_results(p, cfg, nit)
                assert np.all(p.obstacle_terms().cost == 0)
                for k, v in plain.items():
                    assert np.array_equal(v, got[k], equal_nan=True), f"{tag}: {what}: {k} moved ({int(np.sum(v != got[k]))} entries)"
        p.clear_obstacles()
        cl._refused(lambda: p.obstacle_terms(), "the problem has no obstacle terms")
        with generic_pin(not unpinned):   # the planned (cooperative) kernels where they exist
            q.solve_recursive(nit, True, False)
            p.solve_recursive(nit, True, False)
            ms.same(full_results(q, cfg, nit), full_results(p, cfg, nit), f"{tag}: after clear_obstacles")
    finally:
        p.close()
        q.close()


# ------------------------------------------------------------------------------------------------ (c) iterations against the restatement

AL_ROW = dict(row=5, bound=2.0, penalty=0.25)
R_C = 1e-2   # control weight of the cases below: Quu is well conditioned, so K_TOL / D_TOL hold without an allowance for the restatement's own sensitivity
#           (chain, system, T, B, al, iterations)
ITER_CASES = (("panda", "po1", 9, 3, False, 1), ("panda", "po1", 9, 3, False, 3), ("gen4", "pot2", 5, 2, False, 1), ("panda", "po1", 9, 2, True, 1),
              ("panda", "po1", 9, 2, True, 3))


def near_tool(chain, q, obs_row):
    """obs_row = an obstacle of radius 5 cm whose centre lies 6 cm from the tool frame at the joint positions q."""
    pos = cref.link_frames(chain, q[: chain["dof"]])[len(chain["seg_joint"])][1]
    obs_row[:] = [float(pos[0]) + 0.04, float(pos[1]) + 0.02, float(pos[2]) - 0.04, 0.05]


def iter_world(chain, inp, seed):
    """Five spheres, two planes and one set of three obstacles per instance, the first of them near the instance's tool at q0 (so that a pair
    with a gradient is active from the first state on)."""
    rng = np.random.default_rng(seed)
    obs = clr.obstacles_of(len(inp["q0"]), 3, rng)
    for i, q in enumerate(inp["q0"]):
        near_tool(chain, q, obs[i, 0])
    return clr.spheres_of(chain, 5, rng), planes_of(2), obs


def oracle_systems(cfg, inp, cname, B):
    if cfg["kind"] in (capi.SYS_JOINT, capi.SYS_JOINT_TIME):
        return [oracle_system_of_instance(cfg, inp, i) for i in range(B)]
    segs = segs_of(cname)
    return [(oracle_system_of_instance(cfg, inp, i, segs) if segs["dof"] == 7 else nc.oracle_system(cfg, inp, i, segs)) for i in range(B)]


def x0_of(cfg, inp, i, dof):
    nd = cfg["nb_deriv"]
    x = list(inp["q0"][i][:dof]) + (list(inp["dq0"][i][:dof]) if nd == 2 else [])
    return np.array(x + ([0.0] if cfg["kind"] in (capi.SYS_POS_ORN_TIME, capi.SYS_JOINT_TIME) else []))


def check_iterations(ctx, cname, system, T, B, al, nit, tag, weight=20.0):
    cfg, desc, inp, chain = make_problem(ctx, cname, system, T, B, R=R_C, u_scale=0.2)
    dof = chain["dof"]
    sph, pl, obs = iter_world(chain, inp, 31 + T)
    systems = oracle_systems(cfg, inp, cname, B)
    p = workloads.load_batch(ctx, desc, inp, B)
    try:
        p.set_obstacles(sph, pl, obs, MARGIN, weight, 1)
        alr = None
        if al:
            A = np.zeros((1, p.dims.n_x + p.dims.n_u))
            A[0, AL_ROW["row"]] = 1.0
            lam = np.full((B, T - 1, 1), AL_ROW["bound"])
            p.set_constraints(A, np.array([AL_ROW["bound"]]), lam)
            p.solve_al(nit, nit + 1, AL_ROW["penalty"], 1.1, True, False)   # lag_update_step > nb_iter: the multipliers stay
        else:
            p.solve_recursive(nit, True, False)
        K, d, cost, alpha, iters, U = p.K(), p.d(), p.cost(), p.alpha(), p.iters(), p.U()
        trace_alpha = p.trace(nit)[1]
        assert np.any(p.obstacle_terms(want=("cost",)).cost > 0), f"{tag}: no pair is active at the plan"
        worst = dict(K=0.0, d=0.0, cost=0.0)
        for i in range(B):
            world = ref.World(chain, sph, pl, obs[i], MARGIN, weight)
            if al:
                alr = dict(A=A, b=np.array([AL_ROW["bound"]]), lam=lam[i], penalty=AL_ROW["penalty"])
            r = ref.solve(systems[i], workloads.control_weights(cfg, p.dims.n_u), world, x0_of(cfg, inp, i, dof), inp["U0"][i], nit, al=alr)
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


# ------------------------------------------------------------------------------------------------ (d) the term bites

BITE = dict(T=13, nit=12, weight=2000.0, margin=0.06, r_tool=0.05, r_obs=0.08, step=9)


def bite_scenario(ctx):
    """One PosOrn-1 instance on the workloads' Panda, a sphere on the tool, and an obstacle the restated solve WITHOUT the term runs into: its
    centre lies 3 cm beside the tool sphere's centre at step BITE['step'] of that plan.  Returns everything both sides need."""
    cfg, desc, inp, chain = make_problem(ctx, "panda0", "po1", BITE["T"], 1, seed=7, R=R_C, u_scale=0.0)
    s = oracle_systems(cfg, inp, "panda0", 1)[0]
    x0 = x0_of(cfg, inp, 0, 7)
    free = ref.solve(s, workloads.control_weights(cfg, 7), None, x0, inp["U0"][0], BITE["nit"])
    tool = len(chain["seg_joint"]) - 1
    sph = [(tool, (0.0, 0.0, 0.0), BITE["r_tool"])]
    R, pos = cref.link_frames(chain, free["X"][BITE["step"]][:7])[tool + 1]
    centre = np.array([float(pos[0]), float(pos[1]), float(pos[2])]) + np.array([0.0, 0.03, 0.0])
    obs = np.array([[list(centre) + [BITE["r_obs"]]]])
    return cfg, desc, inp, chain, s, x0, sph, obs, free


def clr_min_of(chain, X, sph, obs):
    return float(cref.clearance(chain, X[None, :, :7], sph, [], obs, 1, BITE["margin"], ties=True)["clr_min"][0])


def check_bites_reference(ctx):
    """On (ii) alone: blocked without the term, clear by margin / 2 with it.  Returns the scenario and the restated obstacle solve."""
    sc = bite_scenario(ctx)
    cfg, desc, inp, chain, s, x0, sph, obs, free = sc
    blocked = clr_min_of(chain, free["X"], sph, obs)
    world = ref.World(chain, sph, [], obs[0], BITE["margin"], BITE["weight"])
    avoid = ref.solve(s, workloads.control_weights(cfg, 7), world, x0, inp["U0"][0], BITE["nit"])
    cleared = clr_min_of(chain, avoid["X"], sph, obs)
    print(f"bites: restated clr_min {blocked:.4f} without the term, {cleared:.4f} with it (margin {BITE['margin']})", flush=True)
    assert blocked < 0, f"the scenario does not block the unconstrained plan (clr_min {blocked})"
    assert cleared >= BITE["margin"] / 2, f"the restated solve with the term ends with clr_min {cleared} (< margin / 2)"
    return sc, avoid


def check_bites(ctx):
    sc, avoid = check_bites_reference(ctx)
    cfg, desc, inp, chain, s, x0, sph, obs, free = sc
    rb = capi.clr_robot(sph)
    p = workloads.load_batch(ctx, desc, inp, 1)
    try:
        with generic_pin():
            p.solve_recursive(BITE["nit"], True, False)
            K_free = p.K()
            assert p.clearance(rb, obs, 1, BITE["margin"]).clr_min[0] < 0, "the library's plan without the term is not blocked"
            p.set_obstacles(sph, [], obs, BITE["margin"], BITE["weight"], 1)
            p.solve_recursive(BITE["nit"], True, False)
        got = p.clearance(rb, obs, 1, BITE["margin"])
        assert np.allclose(p.X()[0], avoid["X"], rtol=1e-6, atol=1e-8), "the library's plan with the term is not the restated one"
        assert list(p.trace(BITE["nit"])[1][0]) == avoid["alphas"], "step sizes against the restatement"
        assert got.clr_min[0] >= BITE["margin"] / 2, f"the library's plan with the term has clr_min {got.clr_min[0]}"
        moved = np.abs(p.K() - K_free) / (K_TOL["atol"] + K_TOL["rtol"] * np.abs(K_free))
        assert moved.max() > 100, f"K moves by {moved.max():.3e} tolerances with the term: the check would not see it dropped"
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (e) gains about an obstacle plan

def check_gains(ctx, cname, system, T, B, al, tag):
    cfg, desc, inp, chain = make_problem(ctx, cname, system, T, B, R=R_C)
    sph, pl, obs = iter_world(chain, inp, 77)
    p, q = workloads.load_batch(ctx, desc, inp, B), workloads.load_batch(ctx, desc, inp, B)
    pen = AL_ROW["penalty"]
    try:
        for h in (p, q):
            h.set_obstacles(sph, pl, obs, MARGIN, 20.0, 1)
            if al:
                A = np.zeros((1, h.dims.n_x + h.dims.n_u))
                A[0, AL_ROW["row"]] = 1.0
                h.set_constraints(A, np.array([AL_ROW["bound"]]), np.full((B, T - 1, 1), AL_ROW["bound"]))
        if al:
            p.solve_al(0, 2, pen, 1.0, True, False)
            p.gains_al(pen)
            q.solve_al(1, 2, pen, 1.0, True, False)
        else:
            p.solve_recursive(0, True, False)
            p.gains()
            q.solve_recursive(1, True, False)
        assert np.any(p.obstacle_terms(want=("cost",)).cost > 0), f"{tag}: no pair is active at the plan"
        assert p.K().tobytes() == q.K().tobytes(), f"{tag}: K about the plan differs from the fresh one-iteration solve's"
        assert (q.alpha()[:, None, None] * p.d()).tobytes() == q.d().tobytes(), f"{tag}: d of the solve is not alpha times d about the plan"
        q.clear_obstacles()   # and the terms are in that K: without them it differs
        q.set_controls(inp["U0"])
        (q.solve_al(1, 2, pen, 1.0, True, False) if al else q.solve_recursive(1, True, False))
        assert p.K().tobytes() != q.K().tobytes(), f"{tag}: the gains do not feel the terms"
    finally:
        p.close()
        q.close()


# ------------------------------------------------------------------------------------------------ (f) untouched

def check_untouched(ctx, arrays, tag="untouched"):
    B, T = 13, 9
    cfg = dict(workloads.config("C3"), T=T)
    desc, inp = workloads.make_batch(ctx, cfg, B=B, seed=3)
    chain = clr.chain_of("panda0")
    p = workloads.load_batch(ctx, desc, inp, B)   # C3 carries an AL row: multipliers exist
    sph, pl, obs = iter_world(chain, inp, 5)
    al = cfg["al"]
    try:
        p.set_obstacles(sph, pl, obs, MARGIN, 20.0, 1)
        cl._refused(lambda: p.obstacle_terms(), "ilqr_problem_obstacle_terms needs a plan")
        p.solve_al(0, al["lag"], al["penalty"], al["scaling"], True, False)   # a plan, no gains
        p.obstacle_terms()
        cl._refused(lambda: p.closed_loop(samples=1), "")                     # still no gains: the call did not make any
        p.solve_al(3, 2, al["penalty"], al["scaling"], True, False)
        before = ms.results(p, cfg)
        a = p.obstacle_terms()
        terms_dev(p, arrays)
        ms.same(before, ms.results(p, cfg), f"{tag}: after ilqr_problem_obstacle_terms")
        c1 = p.closed_loop(samples=1)[0]      # the gains of the solve still count
        assert np.all(np.isfinite(c1))
        assert p.obstacle_terms().cost.tobytes() == a.cost.tobytes(), f"{tag}: the same plan, the same terms"
        p.set_controls(inp["U0"])
        cl._refused(lambda: p.obstacle_terms(), "ilqr_problem_obstacle_terms needs a plan")
        p.solve_al(0, al["lag"], al["penalty"], al["scaling"], True, False)
        p.set_obstacles(sph, pl, obs, MARGIN, 20.0, 1)   # a setter: no plan afterwards
        cl._refused(lambda: p.obstacle_terms(), "ilqr_problem_obstacle_terms needs a plan")
        cl._refused(lambda: p.gains(), "ilqr_problem_gains needs a plan")
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (g) refusals

def check_refusals(ctx, arrays, tag="refusals", batch_solvers=True):
    """batch_solvers = False (the host build, which has no batch solver): their refusal is still checked, their acceptance afterwards is not."""
    cfg, desc, inp, chain, sph, pl, obs, tps, w = build(ctx, "gen4")
    B = len(inp["q0"])
    n_seg = len(chain["seg_joint"])
    p = workloads.load_batch(ctx, desc, inp, B)
    L = ctx.L

    def call(rb=None, world=None, weight=1.0, null=(), prob=None, fn="ilqr_problem_set_obstacles"):
        rb = rb if rb is not None else capi.clr_robot(sph, pl)
        world = world if world is not None else capi.ClrWorld(obs.ctypes.data, obs.shape[0], obs.shape[1], tps, MARGIN, 0)
        ctx.check(getattr(L, fn)((prob or p).h, C.byref(rb), C.byref(world) if "world" not in null else None, float(weight)))

    def robot(field, value, i=None, a=None):
        rb = capi.clr_robot(sph, pl)
        if i is None:
            setattr(rb, field, value)
        elif a is None:
            getattr(rb, field)[i] = value
        else:
            getattr(rb, field)[i][a] = value
        return rb

    def world(**kw):
        wd = capi.ClrWorld(obs.ctypes.data, obs.shape[0], obs.shape[1], tps, MARGIN, 0)
        for k, v in kw.items():
            setattr(wd, k, v)
        return wd

    R = cl._refused
    try:
        call()   # the base call is accepted; stats_group = 0 is not read
        R(lambda: call(null=("world",)), "ilqr_problem_set_obstacles: world is a null pointer")
        R(lambda: call(rb=robot("n_sph", 0)), "n_sph must be 1 .. 32 (got 0)")
        R(lambda: call(rb=robot("n_sph", 33)), "n_sph must be 1 .. 32 (got 33)")
        R(lambda: call(rb=robot("sph_link", -2, 0)), "sph_link[0] = -2 is outside -1 .. " + str(n_seg - 1))
        R(lambda: call(rb=robot("sph_link", n_seg - 1, 0)), "sph_link must be non-decreasing")
        R(lambda: call(rb=robot("sph_r", -0.01, 1)), "sph_r[1] must be finite and >= 0")
        R(lambda: call(rb=robot("sph_c", np.nan, 2, 1)), "sph_c[2][1] is not finite")
        R(lambda: call(rb=robot("n_planes", 9)), "n_planes must be 0 .. 8 (got 9)")
        R(lambda: call(rb=robot("plane_n", 0.6 + 1e-8, 1, 0)), "plane_n[1] is not a unit vector")
        R(lambda: call(rb=robot("plane_d", np.nan, 1)), "plane_d[1] is not finite")
        R(lambda: call(world=world(n_obs=-1)), "n_obs must be >= 0 (got -1)")
        R(lambda: call(rb=robot("n_planes", 0), world=world(n_obs=0)), "nothing to keep clear of: n_obs = 0 and n_planes = 0")
        R(lambda: call(world=world(obs=None)), "obs is a null pointer with n_obs = 9")
        R(lambda: call(world=world(traj_per_set=2, n_sets=6)), "is not a multiple of traj_per_set (2)")
        R(lambda: call(world=world(n_sets=12)), "n_sets must be n / traj_per_set = 13 (got 12)")
        R(lambda: call(world=world(margin=np.nan)), "margin is NaN")
        R(lambda: call(world=world(margin=np.inf)), "margin is infinite")
        R(lambda: call(weight=-1.0), "the weight must be finite and >= 0")
        R(lambda: call(weight=np.nan), "the weight must be finite and >= 0")
        R(lambda: call(weight=np.inf), "the weight must be finite and >= 0")
        bad = obs.copy()
        bad[2, 1, 0] = np.nan
        R(lambda: call(world=capi.ClrWorld(bad.ctypes.data, obs.shape[0], obs.shape[1], tps, MARGIN, 0)), "obs[2][1][0] is not finite")
        R(lambda: call(rb=robot("n_sph", 0), fn="ilqr_problem_set_obstacles_dev"), "ilqr_problem_set_obstacles_dev: n_sph must be 1 .. 32")
        # the _dev form copies device to device and gives the same terms
        p.set_obstacles(sph, pl, obs, MARGIN, w, tps)
        p.solve_recursive(0, True, False)
        host = p.obstacle_terms()
        ho = arrays.put(obs)
        p.set_obstacles_dev(capi.clr_robot(sph, pl), capi.ClrWorld(arrays.ptr(ho), obs.shape[0], obs.shape[1], tps, MARGIN, 0), w)
        ctx.synchronize()
        del ho   # no pointer is kept
        p.solve_recursive(0, True, False)
        assert p.obstacle_terms().lxx.tobytes() == host.lxx.tobytes(), f"{tag}: the _dev setter gives other terms"
        R(lambda: p.obstacle_terms(want=()), "every output is a null pointer")
        # a descriptor without a chain
        jcfg = dict(workloads.config("C1j"), T=3)
        jdesc, jinp = workloads.make_batch(ctx, jcfg, B=2)
        pj = workloads.load_batch(ctx, jdesc, jinp, 2)
        try:
            wj = capi.ClrWorld(obs.ctypes.data, 2, obs.shape[1], 1, MARGIN, 0)
            R(lambda: call(rb=capi.clr_robot([(-1, (0.0, 0.0, 0.0), 0.1)]), world=wj, prob=pj), "the descriptor has no chain (n_seg = 0)")
        finally:
            pj.close()
        # the batch solvers refuse a problem that has the terms, and take it again without them
        psi = workloads.psi_of(dict(kind="unitstep", K=2), p.T, p.dims.n_u)
        R(lambda: p.solve_batch_cp(psi, 1, False), "obstacle terms are not supported by the batch solvers")
        R(lambda: p.solve_batch(1, False), "obstacle terms are not supported by the batch solvers")
        p.clear_obstacles()
        if batch_solvers:
            p.solve_batch(1, False)
    finally:
        p.close()
