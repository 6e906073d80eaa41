"""Timing of the obstacle terms of the stage cost (ilqr_problem_set_obstacles), in one session.  Nothing is asserted on a time.
  (a) the derivative pass at the C3 shape (B = 4096 plans of T = 200 steps, a robot of 12 spheres, 8 obstacles shared by all, 1 plane: the world
      of scripts/time_clearance.py): ilqr_problem_obstacle_terms_dev asking for the cost alone, i.e. k_obs_derivs over every (instance, step) and
      the B T doubles k_obs_query copies, beside ilqr_problem_clearance_dev on the same plan and world in the same run;
  (b) a 20-iteration ilqr_solve_al of C3 at B = 256 on the generic kernels (the pin), without and with the terms: what the terms add to the
      kernel set they run on; and the same solve unpinned without the terms: the price of that kernel set (with the terms there is no choice);
  (c) python bench.py --gpus 1 --steps 20 --warmup 3 (plain C3, no obstacle terms) from this tree and, with --parent-tree DIR (a built checkout of
      the parent commit), from that one, three runs each in swapped order.
Every figure of (a), (b) is the HIP-synchronised wall time of the call named: one warm-up outside, then --reps repetitions, median and range.

Usage: python scripts/time_obstacles.py [--reps R] [--parent-tree DIR] [--out profiles/obstacle_timing.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from ilqr_planner_amd import capi, workloads  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--out", default="profiles/obstacle_timing.txt")
args = ap.parse_args()

torch.cuda.init()
ctx = capi.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed_us(fn, reps=args.reps):
    fn()
    ctx.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


cfg = workloads.config("C3")
al = cfg["al"]
B, T = cfg["B"], cfg["T"]
chain = workloads.panda_chain()
n_seg = len(chain["seg_joint"])
rng = np.random.default_rng(7)
links = sorted([-1] + [int(v) for v in rng.integers(0, n_seg, 10)] + [n_seg - 1])
spheres = [(l, rng.uniform(-0.05, 0.05, 3), 0.06) for l in links]
planes = [((0.0, 0.0, 1.0), -0.05)]
robot = capi.clr_robot(spheres, planes)
obs = np.empty((1, 8, 4))
obs[0, :, 0] = rng.uniform(0.2, 0.8, 8)
obs[0, :, 1] = rng.uniform(-0.6, 0.6, 8)
obs[0, :, 2] = rng.uniform(0.1, 0.9, 8)
obs[0, :, 3] = 0.08
MARGIN, WEIGHT = 0.05, 10.0

# (a)
desc, inp = workloads.make_batch(ctx, cfg, B=B)
p = workloads.load_batch(ctx, desc, inp, B)
p.solve_al(3, al["lag"], al["penalty"], al["scaling"], True, False)   # the plan of scripts/time_clearance.py (cooperative kernels)
X = p.X()
p.set_obstacles(robot, None, obs, MARGIN, WEIGHT)
p.set_controls(p.U())
p.solve_al(0, al["lag"], al["penalty"], al["scaling"], True, False)   # the same plan, held by a problem with the terms
ctx.synchronize()
same_plan = np.allclose(p.X(), X, rtol=0, atol=1e-9)
say(f"C3 T = {T}; {robot.n_sph} spheres, {obs.shape[1]} obstacles, {robot.n_planes} plane, margin {MARGIN}, weight {WEIGHT}; median [min .. max] of {args.reps} repetitions after one warm-up, microseconds")
d_obs = torch.from_numpy(obs).cuda()
d_cost = torch.zeros((B, T), dtype=torch.float64, device="cuda")
d_lx = torch.zeros((B, T, 7), dtype=torch.float64, device="cuda")
d_lxx = torch.zeros((B, T, 7, 7), dtype=torch.float64, device="cuda")
d_min = torch.zeros(B, dtype=torch.float64, device="cuda")
d_at = torch.zeros((B, 3), dtype=torch.int32, device="cuda")
d_nb = torch.zeros(B, dtype=torch.int32, device="cuda")
d_el = torch.zeros(B, dtype=torch.int32, device="cuda")
out = capi.ClrOut(None, d_min.data_ptr(), d_at.data_ptr(), d_nb.data_ptr(), d_el.data_ptr(), None)
world = capi.ClrWorld(d_obs.data_ptr(), 1, obs.shape[1], B, MARGIN, 0)
torch.cuda.synchronize()
a1 = timed_us(lambda: p.obstacle_terms_dev(d_cost.data_ptr()))
a2 = timed_us(lambda: p.obstacle_terms_dev(d_cost.data_ptr(), d_lx.data_ptr(), d_lxx.data_ptr()))
a3 = timed_us(lambda: p.clearance_dev(robot, world, out))
say("(a) B = %d: ilqr_problem_obstacle_terms_dev, cost alone (k_obs_derivs + %.1f MB copied)   %9.1f  [%.1f .. %.1f]" % ((B, d_cost.numel() * 8 / 1e6) + a1))
say("(a) ... with lx and lxx (%.1f MB copied)                                               %9.1f  [%.1f .. %.1f]" % (((d_cost.numel() + d_lx.numel() + d_lxx.numel()) * 8 / 1e6,) + a2))
say("(a) ilqr_problem_clearance_dev on the same plan and world, same run                     %9.1f  [%.1f .. %.1f]" % a3)
c = d_cost.cpu().numpy()
say(f"    the plan is that of the solve without the terms: {same_plan}; steps with an active pair: {int(np.sum(c > 0))} of {B * T}; per (instance, step): {a1[0] * 1e3 / (B * T):.2f} ns")
p.close()

# (b)
Bs, NIT = 256, 20
desc, inp = workloads.make_batch(ctx, cfg, B=Bs)
q = workloads.load_batch(ctx, desc, inp, Bs)


def solve():
    q.set_controls(inp["U0"])
    q.reset_multipliers()
    q.solve_al(NIT, al["lag"], al["penalty"], al["scaling"], True, False)


os.environ["ILQR_HIP_PATH"] = "v2"
b0 = timed_us(solve, 5)
os.environ["ILQR_HIP_PATH"] = "v1"
b1 = timed_us(solve, 5)
cost_plain = q.cost()
q.set_obstacles(robot, None, obs, MARGIN, WEIGHT)
b2 = timed_us(solve, 5)
os.environ["ILQR_HIP_PATH"] = "v2"
b3 = timed_us(solve, 5)
say(f"(b) ilqr_solve_al, C3 at B = {Bs}, {NIT} iterations, no early stop; set_controls and reset_multipliers included; 5 repetitions")
say("(b) without the terms, the planned (cooperative) kernels          %11.1f  [%.1f .. %.1f]" % b0)
say("(b) without the terms, pinned to the generic kernels              %11.1f  [%.1f .. %.1f]" % b1)
say("(b) with the terms (generic kernels, pinned)                      %11.1f  [%.1f .. %.1f]" % b2)
say("(b) with the terms, no pin (the plan routes them to the same set) %11.1f  [%.1f .. %.1f]" % b3)
say(f"    with / without on the generic set: {b2[0] / b1[0]:.2f}; generic / cooperative without the terms: {b1[0] / b0[0]:.1f}; mean cost {np.mean(cost_plain):.4f} -> {np.mean(q.cost()):.4f}")
q.close()
ctx.close()

# (c) fresh processes, this tree and the parent's
def bench(tree):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=tree, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} ended with {r.returncode}: {r.stdout[-500:]}{r.stderr[-500:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["ms_per_step"]


order = ["child"] if not args.parent_tree else ["parent", "child", "child", "parent", "parent", "child"]
got = {"parent": [], "child": []}
try:
    for who in order:
        got[who].append(bench(args.parent_tree if who == "parent" else "."))
except Exception as e:   # keep what was measured
    say(f"(c) stopped: {e}")
say("(c) python bench.py --gpus 1 --steps 20 --warmup 3 (plain C3, no obstacle terms), ms_per_step, order " + " ".join(order))
for who in ("parent", "child"):
    if got[who]:
        say(f"(c) {who:6s} {min(got[who]):.4f} .. {max(got[who]):.4f}  mean {np.mean(got[who]):.4f}   [{' '.join('%.4f' % v for v in got[who])}]")
if args.out:
    open(args.out, "w").write("\n".join(lines) + "\n")
