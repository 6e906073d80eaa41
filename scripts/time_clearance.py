"""Timing of the clearance calls (ilqr_problem_clearance, ilqr_clearance_trajectories) at the C3 shape: B = 4096 plans of T = 200 steps, a robot
of 12 spheres, 8 obstacles shared by all and 1 plane.  Every figure is the HIP-synchronised wall time of the call named (one warm-up outside, then
--reps repetitions, each followed by a stream synchronise; median and range), in one session:
  (a) ilqr_problem_clearance_dev on the plan the problem holds (clr_min, clr_at, n_below, eligible);
  (b) ilqr_clearance_trajectories_dev on the S = 64 executions of one ilqr_problem_closed_loop_noise_dev call, X[B][S][T][n_x] left on the device
      (n = B S, traj_per_set = stats_group = S, the same outputs and stats);
  (c) for comparison ilqr_problem_get_X alone: the download that any host-side judgement of the plans must pay before it starts.
The claim to check is only that (a) is below (c).  Not measured: a host-side forward kinematics of the downloaded plans (what (c) would be followed
by), the host forms of the two calls, other sphere and obstacle counts, and the download of the executions (2.9 GB).

Usage: python scripts/time_clearance.py [--reps R] [--samples S] [--out profiles/clearance_timing.txt]"""
import argparse
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from ilqr_planner_amd import capi, workloads  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--samples", type=int, default=64)
ap.add_argument("--out", default="profiles/clearance_timing.txt")
args = ap.parse_args()

torch.cuda.init()
ctx = capi.Context(0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed_us(fn):
    fn()
    ctx.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


cfg = workloads.config("C3")
al = cfg["al"]
B, T, S = cfg["B"], cfg["T"], args.samples
desc, inp = workloads.make_batch(ctx, cfg, B=B)
p = workloads.load_batch(ctx, desc, inp, B)
p.solve_al(3, al["lag"], al["penalty"], al["scaling"], True, False)
ctx.synchronize()
n_x = p.dims.n_x

chain = workloads.panda_chain()
n_seg = len(chain["seg_joint"])
rng = np.random.default_rng(7)
links = sorted([-1] + [int(v) for v in rng.integers(0, n_seg, 10)] + [n_seg - 1])
robot = capi.clr_robot([(l, rng.uniform(-0.05, 0.05, 3), 0.06) for l in links], [((0.0, 0.0, 1.0), -0.05)])
obs = np.empty((1, 8, 4))
obs[0, :, 0] = rng.uniform(0.2, 0.8, 8)
obs[0, :, 1] = rng.uniform(-0.6, 0.6, 8)
obs[0, :, 2] = rng.uniform(0.1, 0.9, 8)
obs[0, :, 3] = 0.08
d_obs = torch.from_numpy(obs).cuda()


def outputs(n, groups):
    t = dict(clr_min=torch.zeros(n, dtype=torch.float64, device="cuda"), clr_at=torch.zeros((n, 3), dtype=torch.int32, device="cuda"),
             n_below=torch.zeros(n, dtype=torch.int32, device="cuda"), eligible=torch.zeros(n, dtype=torch.int32, device="cuda"),
             stats=torch.zeros((max(groups, 1), capi.CLR_STATS), dtype=torch.float64, device="cuda"))
    return t, capi.ClrOut(None, t["clr_min"].data_ptr(), t["clr_at"].data_ptr(), t["n_below"].data_ptr(), t["eligible"].data_ptr(),
                          t["stats"].data_ptr() if groups else None)


say(f"C3 T = {T}, B = {B}; {robot.n_sph} spheres, {obs.shape[1]} obstacles, {robot.n_planes} plane; median [min .. max] of {args.reps} repetitions after one warm-up, microseconds")

# (a) the plan where it lies
ta, out_a = outputs(B, 0)
world_a = capi.ClrWorld(d_obs.data_ptr(), 1, obs.shape[1], B, 0.02, 0)
torch.cuda.synchronize()
a = timed_us(lambda: p.clearance_dev(robot, world_a, out_a))
say("(a) ilqr_problem_clearance_dev, n = B = %d                          %11.1f  [%.1f .. %.1f]" % ((B,) + a))

# (c) the download alone
Xh = np.empty((B, T, n_x))
c = timed_us(lambda: ctx.check(ctx.L.ilqr_problem_get_X(p.h, Xh.ctypes.data)))
say("(c) ilqr_problem_get_X alone (%.1f MB to the host)                    %11.1f  [%.1f .. %.1f]" % ((Xh.nbytes / 1e6,) + c))
say("(a) / (c): %.3f" % (a[0] / c[0]))
host = p.clearance(robot, obs, margin=0.02)
same = all(np.array_equal(getattr(host, f), ta[f].cpu().numpy()) for f in ("clr_min", "clr_at", "n_below", "eligible"))
say(f"the host form returns the same bytes as (a): {same}; plans below the margin: {int(np.sum(host.eligible == 0))} of {B}, lowest clearance {np.min(host.clr_min):.4f}")

# (b) the executions of one closed-loop call, left on the device
Xe = torch.zeros((B, S, T, n_x), dtype=torch.float64, device="cuda")
cost = torch.zeros((B, S), dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
p.closed_loop_noise_dev(S, p.noise(11, sigma_w=0.005, sigma_x0=0.01), None, False, cost.data_ptr(), None, Xe.data_ptr())
ctx.synchronize()
tb, out_b = outputs(B * S, B)
d_obs_b = d_obs.repeat(B, 1, 1).contiguous()   # one set per plan: traj_per_set = S
world_b = capi.ClrWorld(d_obs_b.data_ptr(), B, obs.shape[1], S, 0.02, S)
torch.cuda.synchronize()
b = timed_us(lambda: ctx.clearance_trajectories_dev(desc, B * S, T, Xe.data_ptr(), robot, world_b, out_b))
say("(b) ilqr_clearance_trajectories_dev, n = B S = %d x %d (%.2f GB of X)   %11.1f  [%.1f .. %.1f]" % ((B, S, Xe.numel() * 8 / 1e9) + b))
say("(b) per trajectory: %.3f us; (a) per plan: %.3f us" % (b[0] / (B * S), a[0] / B))
st = tb["stats"].cpu().numpy()
say(f"executions below the margin: {int(np.sum(st[:, 2]))} of {B * S}; with a bad step: {int(np.sum(st[:, 3]))}")
p.close()
ctx.close()
if args.out:
    open(args.out, "w").write("\n".join(lines) + "\n")
