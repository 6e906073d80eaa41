"""Timing of the calls that join instances (ilqr_problem_adopt, ilqr_problem_spread_controls, ilqr_problem_select) and what a multi-start buys.

Shape: C3 (T = 200, one AL row) as G = 256 tasks with S = 16 starts each, B = 4096 instances.  Every figure is the HIP-synchronised wall time
of the calls named (one warm-up, then the median of --reps repetitions, each followed by a stream synchronise), in one session:
  1. the step between the coarse and the polishing solve: select + adopt(CONTROLS | MULTIPLIERS) through the _dev forms, against the composition
     the library offered before -- get_cost, get_U, get_lambda of the B starts, the argmin on the host, set_controls and set_constraints on the
     G tasks.  The ratio is recorded, not asserted.
  2. spread_controls on the B starts, and adopt as the replicator (index b / S, STATE | TARGETS | CONTROLS0) from G tasks to B starts.
  3. what it buys (recorded, not asserted): the whole sequence at a stated sigma_u and coarse_iter -- the share of groups whose winner is not
     member 0, and the winner's coarse cost against member 0's.

Usage: python scripts/time_multistart.py [--reps R] [--out profiles/multistart_timing.txt]"""
import argparse
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from ilqr_planner_amd import capi, workloads  # noqa: E402

G, S, SEED, SIGMA_U, COARSE, REFINE = 256, 16, 2024, 0.3, 3, 5
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default="profiles/multistart_timing.txt")
args = ap.parse_args()

torch.cuda.init()
ctx = capi.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median_us(fn):
    fn()
    ctx.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def final_penalty(n, al):
    pen = al["penalty"]
    for it in range(n):
        if (it + 1) % al["lag"] == 0:
            pen *= al["scaling"]
    return pen


cfg = workloads.config("C3")
al = cfg["al"]
B = G * S
desc, inp = workloads.make_batch(ctx, cfg, B=G)
T, nu = cfg["T"], inp["U0"].shape[2]
tasks = workloads.load_batch(ctx, desc, inp, G)
starts = capi.BatchProblem(ctx, desc, B)
starts.set_constraints(inp["A"], inp["b"], np.repeat(inp["lambda0"], S, axis=0))
rep = torch.from_numpy((np.arange(B) // S).astype(np.int32)).cuda()
winner = torch.zeros(G, dtype=torch.int32, device="cuda")
best = torch.zeros(G, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
say(f"C3 T = {T}: G = {G} tasks, S = {S} starts each, B = {B} instances; median [min .. max] of {args.reps} repetitions after one warm-up, microseconds")

# 2. the replicator and the spread
REPL = capi.ADOPT_STATE | capi.ADOPT_TARGETS | capi.ADOPT_CONTROLS0
say("adopt_dev(index b / S, STATE | TARGETS | CONTROLS0), G -> B      %9.1f  [%.1f .. %.1f]" % median_us(lambda: starts.adopt_dev(tasks, rep.data_ptr(), REPL)))
say("spread_controls(S, seed, sigma_u = %.2g) on B                    %9.1f  [%.1f .. %.1f]" % ((SIGMA_U,) + median_us(lambda: starts.spread_controls_dev(S, SEED, SIGMA_U))))

# the coarse solve from one spread
starts.adopt_dev(tasks, rep.data_ptr(), REPL)
starts.spread_controls(S, SEED, SIGMA_U)
starts.solve_al(COARSE, al["lag"], al["penalty"], al["scaling"], True, False)
ctx.synchronize()

# 1. winners into the task problem
PLAN = capi.ADOPT_CONTROLS | capi.ADOPT_MULTIPLIERS


def on_device():
    starts.select_dev(S, None, None, winner.data_ptr(), best.data_ptr(), None)
    tasks.adopt_dev(starts, winner.data_ptr(), PLAN)


def on_host():
    cost, U, lam = starts.cost(), starts.U(), starts.lam()
    w = np.arange(G) * S + np.argmin(np.where(np.isfinite(cost), cost, np.inf).reshape(G, S), axis=1)
    tasks.set_controls(U[w])
    tasks.set_constraints(inp["A"], inp["b"], lam[w])


dev = median_us(on_device)
host = median_us(on_host)
say("select_dev + adopt_dev(CONTROLS | MULTIPLIERS), B -> G           %9.1f  [%.1f .. %.1f]" % dev)
say("get_cost, get_U, get_lambda, host argmin, set_controls, set_constraints  %9.1f  [%.1f .. %.1f]" % host)
say("ratio host / device: %.1f" % (host[0] / dev[0]))
w_dev = winner.cpu().numpy()
cost = starts.cost()
w_host = np.arange(G) * S + np.argmin(np.where(np.isfinite(cost), cost, np.inf).reshape(G, S), axis=1)
say(f"the two pick the same winners: {bool(np.array_equal(w_dev, w_host))}")

# 3. what it buys
sel = starts.select(S)
first = starts.get_at(np.arange(G) * S, want_X=False, want_U=False, want_iters=False, want_status=False).cost
tasks.adopt(starts, sel.winner, PLAN)
tasks.solve_al(REFINE, al["lag"], final_penalty(COARSE, al), al["scaling"], True, False)
multi = tasks.cost()
single = workloads.load_batch(ctx, desc, inp, G)
single.solve_al(COARSE, al["lag"], al["penalty"], al["scaling"], True, False)
plain = workloads.load_batch(ctx, desc, inp, G)
plain.adopt(single, np.arange(G), PLAN)
plain.solve_al(REFINE, al["lag"], final_penalty(COARSE, al), al["scaling"], True, False)
alone = plain.cost()
say(f"sigma_u = {SIGMA_U}, coarse_iter = {COARSE}, then {REFINE} iterations: winner is not member 0 in {np.mean(sel.winner % S != 0):.3f} of the groups; "
    f"candidates per group {sel.n_candidates.min()} .. {sel.n_candidates.max()}")
say(f"coarse cost, mean over the groups: winner {np.mean(sel.best):.6g}, member 0 {np.mean(first):.6g}; median ratio winner / member 0 {np.median(sel.best / first):.4f}")
say(f"polished cost, mean over the tasks: multi-start {np.mean(multi):.6g}, the single start continued alike {np.mean(alone):.6g}; "
    f"multi-start is lower for {np.mean(multi < alone):.3f} of the tasks, equal for {np.mean(multi == alone):.3f}")
for q in (tasks, starts, single, plain):
    q.close()
ctx.close()
if args.out:
    open(args.out, "w").write("\n".join(lines) + "\n")
