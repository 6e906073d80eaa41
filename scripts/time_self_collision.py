"""Timing of self-collision pairs in the clearance calls and the obstacle terms, in one session.  Nothing is asserted on a time.
The world of scripts/time_clearance.py and scripts/time_obstacles_coop.py at the C3 shape (T = 200, 12 spheres, 8 obstacles shared by all,
1 plane), with 0 and with 16 self pairs on 4 anchors:
  (a) ilqr_problem_clearance_dev on the plan of a 0-iteration solve at B = 4096 (k_clr_plan, k_clr_fold);
  (b) ilqr_problem_obstacle_terms_dev on the same plan (k_obs_derivs, k_obs_query);
  (c) ilqr_solve_al with 20 iterations on the cooperative path at B = 256 and B = 4096, set_controls and reset_multipliers included.
Every figure is the HIP-synchronised wall time of the call named: one warm-up outside, then the repetitions, median [min .. max].
Run from a built checkout of the parent commit (whose clr_robot has no self_pairs keyword) the script measures the 0-pair figures alone: they
are the yardstick the 0-pair figures of this tree are read against.

Usage: python scripts/time_self_collision.py [--reps R] [--out profiles/self_collision_timing.txt]   (the tree measured is the working directory's)"""
import argparse
import inspect
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from ilqr_planner_amd import capi, workloads  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()

torch.cuda.init()
ctx = capi.Context(0)
lines = []
HAS_PAIRS = "self_pairs" in inspect.signature(capi.clr_robot).parameters


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed_ms(fn, reps=args.reps):
    fn()
    ctx.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


cfg = workloads.config("C3")
al = cfg["al"]
T = cfg["T"]
chain = workloads.panda_chain()
n_seg = len(chain["seg_joint"])
rng = np.random.default_rng(7)
links = sorted([-1] + [int(v) for v in rng.integers(0, n_seg, 10)] + [n_seg - 1])
spheres = [(l, rng.uniform(-0.05, 0.05, 3), 0.06) for l in links]
planes = [((0.0, 0.0, 1.0), -0.05)]
obs = np.empty((1, 8, 4))
obs[0, :, 0] = rng.uniform(0.2, 0.8, 8)
obs[0, :, 1] = rng.uniform(-0.6, 0.6, 8)
obs[0, :, 2] = rng.uniform(0.1, 0.9, 8)
obs[0, :, 3] = 0.08
MARGIN, WEIGHT, NIT = 0.05, 10.0, 20


def moves(la, lb):
    return any(int(chain["seg_joint"][s]) >= 0 for s in range(la + 1, lb + 1))


every = [(a, b) for a in range(len(spheres)) for b in range(a + 1, len(spheres)) if moves(spheres[a][0], spheres[b][0])]
anchors = sorted({a for a, _ in every})[:4]
pairs = [p for a in anchors for p in [q for q in reversed(every) if q[0] == a][:4]]   # each anchor against its four farthest partners
assert len(pairs) == 16, f"{len(pairs)} pairs"
robots = {0: capi.clr_robot(spheres, planes)}
if HAS_PAIRS:
    robots[16] = capi.clr_robot(spheres, planes, self_pairs=pairs)
say(f"C3 T = {T}; {len(spheres)} spheres, {obs.shape[1]} obstacles, {len(planes)} plane, margin {MARGIN}, weight {WEIGHT}; self pairs: "
    f"{sorted(robots)}; median [min .. max] of {args.reps} repetitions after one warm-up, milliseconds")

for B in (256, 4096):
    desc, inp = workloads.make_batch(ctx, cfg, B=B)
    q = workloads.load_batch(ctx, desc, inp, B)
    d_obs = torch.from_numpy(obs).cuda()
    world = capi.ClrWorld(d_obs.data_ptr(), 1, obs.shape[1], B, MARGIN, 0)
    d_min = torch.empty(B, dtype=torch.float64, device="cuda")
    d_el = torch.empty(B, dtype=torch.int32, device="cuda")
    out = capi.ClrOut(None, d_min.data_ptr(), None, None, d_el.data_ptr(), None)
    d_cost = torch.empty((B, T), dtype=torch.float64, device="cuda")
    d_lx = torch.empty((B, T, 7), dtype=torch.float64, device="cuda")
    d_lxx = torch.empty((B, T, 7, 7), dtype=torch.float64, device="cuda")

    def solve():
        q.set_controls(inp["U0"])
        q.reset_multipliers()
        q.solve_al(NIT, al["lag"], al["penalty"], al["scaling"], True, False)

    for n_self, robot in robots.items():
        q.set_obstacles(robot, None, obs, MARGIN, WEIGHT)
        if B == 4096:
            q.set_controls(inp["U0"])
            q.solve_al(0, al["lag"], al["penalty"], al["scaling"], True, False)
            t = timed_ms(lambda: q.clearance_dev(robot, world, out))
            say(f"(a) ilqr_problem_clearance_dev, B = {B}, {n_self:2d} self pairs           %9.3f  [%.3f .. %.3f]" % t)
            t = timed_ms(lambda: q.obstacle_terms_dev(d_cost.data_ptr(), d_lx.data_ptr(), d_lxx.data_ptr()))
            say(f"(b) ilqr_problem_obstacle_terms_dev, B = {B}, {n_self:2d} self pairs      %9.3f  [%.3f .. %.3f]" % t)
        ctx.set_obstacle_path("cooperative")
        t = timed_ms(solve)
        ctx.set_obstacle_path("generic")
        say(f"(c) ilqr_solve_al, cooperative path, B = {B}, {NIT} iterations, {n_self:2d} self pairs  %9.2f  [%.2f .. %.2f]   mean cost {np.mean(q.cost()):.6f}" % t)
    q.close()
ctx.close()
if args.out:
    open(args.out, "w").write("\n".join(lines) + "\n")
