"""Timing of ilqr_problem_gains_al and what its gains are for.

Call time: the HIP-synchronised wall time of a call (a warm-up, then --reps calls, each followed by a stream synchronise) at C3 B = 4096 after
solve_al, C4 B = 4096 with the one row of the AL workloads (q_6 <= 2.0) after solve_al, and the C5 shape B = 8192 with that row after a Batch-CP
solve.  The yardstick is the solver's own sweep at the same shape in the same session: ILQR_PROF_OTHER + ILQR_PROF_BACKWARD per iteration of
ilqr_solve_al under ilqr_profile_enable (one stream, one kernel at a time).  The profiled call itself is shown too (its launches per category).

What the gains are for (recorded, not asserted): on the C3 AL workload, closed_loop_report_con (S = 64, the noise of scripts/time_closed_loop_con.py)
and closed_loop_cov_con on gains() and on gains_al(final penalty) of the same plan, side by side.

Usage: python scripts/time_gains_al.py [--reps R] [--out profiles/gains_al_timing.txt]"""
import argparse
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from ilqr_planner_amd import capi, workloads  # noqa: E402

PROF = dict(rollout=0, backward=1, forward=2, other=3, apply=4)
AL = dict(row=5, bound=2.0, penalty=0.25, scaling=1.1, lag=5)   # the row and schedule of the AL workloads
SW, SX0, CON_TOL, S, SEED = 1e-3, 1e-2, 0.0, 64, 2024             # scripts/time_closed_loop_con.py
KP_TOL, LIM_TOL = [0.02, 0.1, -1, -1, -1], 0.0
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default="profiles/gains_al_timing.txt")
args = ap.parse_args()

ctx = capi.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def final_penalty(n, al):
    pen = al["penalty"]
    for it in range(n):
        if (it + 1) % al["lag"] == 0:
            pen *= al["scaling"]
    return pen


def wall_us(p, pen):
    p.gains_al(pen)
    ctx.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        p.gains_al(pen)
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


say(f"ilqr_problem_gains_al, wall time of a call + stream synchronise, median and minimum of {args.reps}; yardstick: OTHER + BACKWARD per iteration of")
say("a profiled ilqr_solve_al(5 iterations, lag 5, line search, no early stop) at the same shape")
for name, B in (("C3", 4096), ("C4", 4096), ("C5", 8192)):
    cfg = workloads.config(name)
    T = cfg["T"]
    al = cfg.get("al", AL)
    desc, inp = workloads.make_batch(ctx, cfg, B=B)
    p = workloads.load_batch(ctx, desc, inp, B)
    if "A" not in inp:
        A = np.zeros((1, p.dims.n_x + p.dims.n_u))
        A[0, al["row"]] = 1.0
        p.set_constraints(A, np.array([al["bound"]]), np.full((B, T - 1, 1), al["bound"]))
    nit = 5
    ctx.profile(True)
    p.solve_al(nit, al["lag"], al["penalty"], al["scaling"], True, False)
    ctx.synchronize()
    ctx.profile_reset()
    p.reset_multipliers()
    p.solve_al(nit, al["lag"], al["penalty"], al["scaling"], True, False)
    ctx.synchronize()
    t = {k: ctx.profile_get(v) for k, v in PROF.items()}
    yard = (t["other"][0] + t["backward"][0]) / nit * 1e3
    pen = final_penalty(nit, al)
    ctx.profile_reset()
    p.gains_al(pen)
    ctx.synchronize()
    g = {k: ctx.profile_get(v) for k, v in PROF.items()}
    ctx.profile(False)
    ctx.profile_reset()
    if cfg["solver"] == "batch_cp":
        p.solve_batch_cp(workloads.psi_of(cfg["psi"], T, p.dims.n_u), 3, False)
        src = "after a Batch-CP solve"
    else:
        p.reset_multipliers()
        p.solve_al(nit, al["lag"], al["penalty"], al["scaling"], True, False)
        src = "after solve_al"
    ctx.synchronize()
    med, best = wall_us(p, pen)
    say(f"{name} T={T} B={B}: gains_al {med:9.1f} us (min {best:9.1f}) {src}; solver's OTHER + BACKWARD {yard:9.1f} us per iteration "
        f"(other {t['other'][0] / nit * 1e3:.1f}, backward {t['backward'][0] / nit * 1e3:.1f}); ratio {med / yard:.2f}; profiled gains_al call: other "
        f"{g['other'][0] * 1e3:.1f} us in {g['other'][1]} launches, backward {g['backward'][0] * 1e3:.1f} us in {g['backward'][1]}, rollout/forward/apply "
        f"launches {g['rollout'][1]}/{g['forward'][1]}/{g['apply'][1]}")
    p.close()

# ---- what the gains are for
cfg = workloads.config("C3")
B, al, nit = 4096, cfg["al"], cfg["nb_iter"]
desc, inp = workloads.make_batch(ctx, cfg, B=B)
p = workloads.load_batch(ctx, desc, inp, B)
p.solve_al(nit, al["lag"], al["penalty"], al["scaling"], True, False)
pen = final_penalty(nit, al)
lam = p.lam()
g_plan = p.X()[:, :-1, al["row"]] - al["bound"]
say("")
say(f"C3 T={cfg['T']} B={B} after solve_al({nit}, lag {al['lag']}, penalty {al['penalty']}, scaling {al['scaling']}): final penalty {pen:.6g}; the plan's own rows: "
    f"max g {g_plan.max():.3e}, instances with g > 0 somewhere {int((g_plan.max(axis=1) > 0).sum())}, with lambda > 0 somewhere {int((lam.max(axis=(1, 2)) > 0).sum())}")
say(f"closed_loop_report_con(con_tol {CON_TOL}, S = {S}, sigma_w {SW}, sigma_x0 {SX0}, kp_tol {KP_TOL}, lim_tol {LIM_TOL}) and closed_loop_cov_con, batch means")
for law, call in (("gains()", p.gains), (f"gains_al({pen:.6g})", lambda: p.gains_al(pen))):
    call()
    for ff in (False, True):
        r = p.closed_loop_report_con(CON_TOL, samples=S, seed=SEED, sigma_w=SW, sigma_x0=SX0, with_feedforward=ff, kp_tol=KP_TOL, lim_tol=LIM_TOL)
        cs, oc = r.con_stats, r.outcome_con
        say(f"{law:22s} ff={int(ff)}: con_stats mean con_max {np.nanmean(cs[:, 0]):+.4e}, max con_max {np.nanmax(cs[:, 1]):+.4e}, mean con_steps {np.nanmean(cs[:, 2]):.3f}, "
            f"n_con / (B S) {cs[:, 4].sum() / (B * S):.4f}, bad {int(cs[:, 5].sum())}; outcome_con ok/miss/lim/con/bad per (B S) "
            f"{' / '.join(f'{oc[:, j].sum() / (B * S):.4f}' for j in range(5))}; cost mean {np.nanmean(r.stats[:, 0]):.6e}, variance {np.nanmean(r.stats[:, 1]):.3e}, "
            f"max {np.nanmax(r.stats[:, 3]):.6e}")
    c = p.closed_loop_cov_con(SW, SX0)
    z = c.con_z[np.isfinite(c.con_z)]
    say(f"{law:22s} cov : con_z median {np.median(z):+.3f}, 5 % quantile {np.quantile(z, 0.05):+.3f}, min {z.min():+.3f}, negative {int((z < 0).sum())} of {len(z)} finite; "
        f"largest con_var {np.nanmax(c.con_var):.3e}")
p.close()
ctx.close()
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
