"""Timing of the obstacle terms on the cooperative kernels (ilqr_ctx_set_obstacle_path(COOPERATIVE)), in one session.  Nothing is asserted on a time.
  (a) the world of scripts/time_obstacles.py at the C3 shape (T = 200, 12 spheres, 8 obstacles shared by all, 1 plane), ilqr_solve_al with 20
      iterations: at B = 256 the cooperative mode against the generic mode of the same library; at B = 4096 the cooperative mode alone, with the
      per-category split of the context's per-launch profile (ilqr_profile_enable: one kernel at a time);
  (b) the multi-start shape: 256 tasks x 16 starts = 4096 starts of C3 with the terms on both problems, cooperative, end to end (adopt, spread,
      coarse solves, clearance, select, adopt, polishing solve), through capi.py;
  (c) python bench.py --gpus 1 --steps 20 --warmup 3 (plain C3, no obstacle terms) from this tree and, with --parent-tree DIR (a built checkout of
      the parent commit), from that one, three runs each in alternating order.
Every figure of (a), (b) is the HIP-synchronised wall time of the call named: one warm-up outside, then the repetitions, median and range.

Usage: python scripts/time_obstacles_coop.py [--reps R] [--skip-generic] [--parent-tree DIR] [--out profiles/obstacle_coop_timing.txt]"""
import argparse
import json
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from ilqr_planner_amd import capi, workloads  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip-generic", action="store_true", help="leave out the generic-mode solve of (a): seconds per repetition")
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--out", default="profiles/obstacle_coop_timing.txt")
args = ap.parse_args()

torch.cuda.init()
ctx = capi.Context(0)
lines = []


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
robot = capi.clr_robot(spheres, planes)
obs = np.empty((1, 8, 4))
obs[0, :, 0] = rng.uniform(0.2, 0.8, 8)
obs[0, :, 1] = rng.uniform(-0.6, 0.6, 8)
obs[0, :, 2] = rng.uniform(0.1, 0.9, 8)
obs[0, :, 3] = 0.08
MARGIN, WEIGHT, NIT = 0.05, 10.0, 20
PROF = ("rollout", "backward", "forward", "other", "apply")
say(f"C3 T = {T}; {robot.n_sph} spheres, {obs.shape[1]} obstacles, {robot.n_planes} plane, margin {MARGIN}, weight {WEIGHT}; "
    f"median [min .. max] of {args.reps} repetitions after one warm-up, milliseconds")

# (a)
res = {}
for B in (256, 4096):
    desc, inp = workloads.make_batch(ctx, cfg, B=B)
    q = workloads.load_batch(ctx, desc, inp, B)

    def solve():
        q.set_controls(inp["U0"])
        q.reset_multipliers()
        q.solve_al(NIT, al["lag"], al["penalty"], al["scaling"], True, False)

    t_plain = timed_ms(solve)
    cost_plain = q.cost()
    q.set_obstacles(robot, None, obs, MARGIN, WEIGHT)
    ctx.set_obstacle_path("cooperative")
    t_coop = timed_ms(solve)
    cost_coop, alpha_coop = q.cost(), q.trace(NIT)[1]
    say(f"(a) ilqr_solve_al, C3 at B = {B}, {NIT} iterations, no early stop; set_controls and reset_multipliers included")
    say("(a) without the terms (the planned cooperative kernels)   %11.2f  [%.2f .. %.2f]" % t_plain)
    say("(a) with the terms, cooperative mode                      %11.2f  [%.2f .. %.2f]" % t_coop)
    say(f"    mean cost {np.mean(cost_plain):.4f} -> {np.mean(cost_coop):.4f}; accepted step sizes below 1: {int(np.sum(alpha_coop < 1))} of {alpha_coop.size}; "
        f"per iteration with the terms: {t_coop[0] / NIT:.3f} ms")
    if B == 256 and not args.skip_generic:
        ctx.set_obstacle_path("generic")
        t_gen = timed_ms(solve, 3)
        cost_gen = q.cost()
        say("(a) with the terms, generic mode (3 repetitions)          %11.2f  [%.2f .. %.2f]" % t_gen)
        say(f"    generic / cooperative: {t_gen[0] / t_coop[0]:.1f}; the parent's recorded figure for this solve: 3341 ms; "
            f"worst relative cost difference between the modes {float(np.max(np.abs(cost_gen - cost_coop) / np.abs(cost_gen))):.2e}")
        ctx.set_obstacle_path("cooperative")
    if B == 4096:
        ctx.profile(True)
        ctx.profile_reset()
        solve()
        ctx.synchronize()
        split = [ctx.profile_get(i) for i in range(len(PROF))]
        ctx.profile(False)
        say("(a) per-launch profile of one such solve (one kernel at a time), ms (launch groups): " +
            ", ".join(f"{n} {ms:.2f} ({k})" for n, (ms, k) in zip(PROF, split)) + f"; sum {sum(ms for ms, _ in split):.2f}")
        say("    rollout: k_init_roll_lti, k_init_finish, k_obs_ls (initial cost), k_al_post; other: k_kp_derivs, k_obs_derivs, k_stage_dense; backward: "
            "k_backward_si_dpp<.., SW_DENSE>; forward: the rollout, k_obs_ls + k_obs_ls_sum, k_select; apply: k_apply, k_flip_ran")
    ctx.set_obstacle_path("generic")
    q.close()

# (b)
G, S, COARSE, POLISH = 256, 16, 3, 10
B = G * S
desc, inp = workloads.make_batch(ctx, cfg, B=G)
tasks = workloads.load_batch(ctx, desc, inp, G)
starts = capi.BatchProblem(ctx, desc, B)
starts.set_constraints(inp["A"], inp["b"], np.repeat(inp["lambda0"], S, axis=0))
rep = (np.arange(B) // S).astype(np.int32)
sigma = np.full(7, 0.3)
obs_g = np.repeat(obs, G, axis=0)
out = {}


def multistart():
    tasks.set_controls(inp["U0"])
    tasks.reset_multipliers()
    starts.adopt(tasks, rep, capi.ADOPT_STATE | capi.ADOPT_TARGETS | capi.ADOPT_CONTROLS0)
    starts.reset_multipliers()
    starts.spread_controls(S, 4711, sigma)
    starts.set_obstacles(robot, None, obs_g, MARGIN, WEIGHT, S)
    tasks.set_obstacles(robot, None, obs_g, MARGIN, WEIGHT, 1)
    starts.solve_al(COARSE, al["lag"], al["penalty"], al["scaling"], True, False)
    c = starts.clearance(robot, obs_g, S, MARGIN, want=("clr_min", "eligible"))
    sel = starts.select(S, None, c.eligible)
    tasks.adopt(starts, sel.winner, capi.ADOPT_CONTROLS | capi.ADOPT_MULTIPLIERS)
    tasks.solve_al(POLISH, al["lag"], al["penalty"], al["scaling"], True, False)
    out["n"] = sel.n_candidates


ctx.set_obstacle_path("cooperative")
t_ms = timed_ms(multistart)
say(f"(b) multi-start, {G} tasks x {S} starts = {B} starts of C3 with the terms, cooperative mode, {COARSE} coarse + {POLISH} polishing AL iterations, end to end")
say("(b) adopt, spread, set_obstacles, coarse solves, clearance, select, adopt, polish   %11.2f  [%.2f .. %.2f]" % t_ms)
say(f"    groups with a candidate: {int(np.sum(out['n'] > 0))} of {G}")
ctx.set_obstacle_path("generic")
tasks.close()
starts.close()
ctx.close()


# (c) fresh processes, this tree and the parent's
def bench(tree):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=tree, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} ended with {r.returncode}: {r.stdout[-500:]}{r.stderr[-500:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["ms_per_step"]


order = ["child"] if not args.parent_tree else ["parent", "child", "parent", "child", "parent", "child"]
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
