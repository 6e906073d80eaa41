"""Timing of ilqr_problem_gains: the HIP-synchronised wall time of a call (a warm-up, then --reps calls, each followed by a stream
synchronise) at C3 B = 4096, the C5 shape B = 8192 after a Batch-CP solve, and C4 B = 4096.
The yardstick is the solver's own sweep at the same shape in the same session: ILQR_PROF_OTHER + ILQR_PROF_BACKWARD per iteration of
ilqr_solve_recursive under ilqr_profile_enable (one stream, one kernel at a time) -- a gains call runs that pair and k_gains_prepare, nothing else.
The profiled call itself is shown too (its launches per category).
Usage: python scripts/time_gains.py [--reps R] [--out profiles/gains_timing.txt]"""
import argparse
import sys
import time

sys.path.insert(0, ".")
from ilqr_planner_amd import capi, workloads  # noqa: E402

PROF = dict(rollout=0, backward=1, forward=2, other=3, apply=4)
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default="profiles/gains_timing.txt")
args = ap.parse_args()

ctx = capi.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def wall_us(p):
    p.gains()
    ctx.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        p.gains()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


say(f"ilqr_problem_gains, wall time of a call + stream synchronise, median and minimum of {args.reps}; yardstick: OTHER + BACKWARD per iteration of")
say("a profiled ilqr_solve_recursive(5 iterations, line search, no early stop) at the same shape")
for name, B in (("C3", 4096), ("C5", 8192), ("C4", 4096)):
    cfg = workloads.config(name)
    T = cfg["T"]
    desc, inp = workloads.make_batch(ctx, cfg, B=B)
    inp.pop("A", None)  # the yardstick is the plain sweep: no constraint rows
    p = workloads.load_batch(ctx, desc, inp, B)
    nit = 5
    ctx.profile(True)
    p.solve_recursive(nit, True, False)
    ctx.synchronize()
    ctx.profile_reset()
    p.solve_recursive(nit, True, False)
    ctx.synchronize()
    t = {k: ctx.profile_get(v) for k, v in PROF.items()}
    yard = (t["other"][0] + t["backward"][0]) / nit * 1e3
    ctx.profile_reset()
    p.gains()
    ctx.synchronize()
    g = {k: ctx.profile_get(v) for k, v in PROF.items()}
    ctx.profile(False)
    ctx.profile_reset()
    if cfg["solver"] == "batch_cp":
        p.solve_batch_cp(workloads.psi_of(cfg["psi"], T, p.dims.n_u), 3, False)
        src = "after a Batch-CP solve"
    else:
        p.solve_recursive(3, True, False)
        src = "after a Riccati solve"
    ctx.synchronize()
    med, best = wall_us(p)
    say(f"{name} T={T} B={B}: gains {med:9.1f} us (min {best:9.1f}) {src}; solver's OTHER + BACKWARD {yard:9.1f} us per iteration "
        f"(other {t['other'][0] / nit * 1e3:.1f}, backward {t['backward'][0] / nit * 1e3:.1f}); profiled gains call: other {g['other'][0] * 1e3:.1f} us in "
        f"{g['other'][1]} launches, backward {g['backward'][0] * 1e3:.1f} us in {g['backward'][1]}, rollout/forward/apply launches "
        f"{g['rollout'][1]}/{g['forward'][1]}/{g['apply'][1]}")
    p.close()
ctx.close()
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
