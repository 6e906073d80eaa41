"""Timing of ilqr_problem_closed_loop_cov_clr at the C3 shape: B = 4096 plans of T = 200 steps, a robot of 12 spheres, 8 obstacles shared by all
and 1 plane (the shape of profiles/clearance_timing.txt).  Every figure is the HIP-synchronised wall time of the call named (one warm-up outside,
then --reps repetitions, each followed by a stream synchronise; median and range), in one session:
  (1) ilqr_problem_closed_loop_cov_clr_dev asking for clr_z_min only (Sigma goes to the context's buffer);
  (2) the same call's covariance part alone: ilqr_problem_closed_loop_cov_dev asking for lim_z;
  (3) the sampled route it replaces at S = 64: ilqr_problem_closed_loop_noise_dev with X left on the device, then
      ilqr_clearance_trajectories_dev with stats (n = B S, traj_per_set = stats_group = S).
The only claim to check is that (1) is below (3).  Not measured: a transposed copy of Sigma for k_cov_clr's reads (the plain form only), other
sphere and obstacle counts, the host forms.

Usage: python scripts/time_cov_clearance.py [--reps R] [--samples S] [--out profiles/cov_clearance_timing.txt]"""
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
ap.add_argument("--out", default="profiles/cov_clearance_timing.txt")
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
SW, SX, MARGIN, Z_TOL = 0.005, 0.01, 0.02, 3.0

say(f"C3 T = {T}, B = {B}; {robot.n_sph} spheres, {obs.shape[1]} obstacles, {robot.n_planes} plane; sigma_w = {SW}, sigma_x0 = {SX}; median [min .. max] of {args.reps} "
    "repetitions after one warm-up, microseconds")

# (1) the analytic call, clr_z_min only
zmin = torch.zeros(B, dtype=torch.float64, device="cuda")
world = capi.ClrWorld(d_obs.data_ptr(), 1, obs.shape[1], B, MARGIN, 0)
ck = capi.ClCovClr(None, None, zmin.data_ptr(), None, None)
torch.cuda.synchronize()
t1 = timed_us(lambda: p.closed_loop_cov_clr_dev(SW, SX, robot, world, Z_TOL, ck))
say("(1) ilqr_problem_closed_loop_cov_clr_dev, clr_z_min only                    %11.1f  [%.1f .. %.1f]" % t1)

# (2) its covariance part alone
lim_z = torch.zeros(B, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
t2 = timed_us(lambda: p.closed_loop_cov_dev(SW, SX, lim_z_ptr=lim_z.data_ptr()))
say("(2) ilqr_problem_closed_loop_cov_dev, lim_z only                            %11.1f  [%.1f .. %.1f]" % t2)
say("(1) - (2): %.1f us for Sigma's stores, k_cov_clr and k_cov_clr_fold" % (t1[0] - t2[0]))

# (3) the sampled route at S samples
Xe = torch.zeros((B, S, T, n_x), dtype=torch.float64, device="cuda")
cost = torch.zeros((B, S), dtype=torch.float64, device="cuda")
nz = p.noise(11, sigma_w=SW, sigma_x0=SX)
n = B * S
out = dict(clr_min=torch.zeros(n, dtype=torch.float64, device="cuda"), stats=torch.zeros((B, capi.CLR_STATS), dtype=torch.float64, device="cuda"))
co = capi.ClrOut(None, out["clr_min"].data_ptr(), None, None, None, out["stats"].data_ptr())
d_obs_b = d_obs.repeat(B, 1, 1).contiguous()   # one set per plan: traj_per_set = S
world_b = capi.ClrWorld(d_obs_b.data_ptr(), B, obs.shape[1], S, MARGIN, S)
torch.cuda.synchronize()


def sampled():
    p.closed_loop_noise_dev(S, nz, None, False, cost.data_ptr(), None, Xe.data_ptr())
    ctx.clearance_trajectories_dev(desc, n, T, Xe.data_ptr(), robot, world_b, co)


t3 = timed_us(sampled)
say("(3) closed_loop_noise_dev + clearance_trajectories_dev, S = %d (%.2f GB of X) %11.1f  [%.1f .. %.1f]" % ((S, Xe.numel() * 8 / 1e9) + t3))
say("(1) / (3): %.4f" % (t1[0] / t3[0]))

# what the two routes say: the share of executions below the margin against the normal tail at the plan's clr_z_min
st = out["stats"].cpu().numpy()
z = zmin.cpu().numpy()
say(f"plans with clr_z_min < {Z_TOL}: {int(np.sum(z < Z_TOL))} of {B}; plans with an execution below the margin: {int(np.sum(st[:, 2] > 0))}; bad steps: {int(np.sum(np.isnan(z)))}")
host = p.closed_loop_cov_clr(SW, SX, robot, (obs, B, MARGIN), Z_TOL, want=("clr_z_min",))
say(f"the host form returns the same bytes as (1): {host.clr_z_min.tobytes() == z.tobytes()}")
p.close()
ctx.close()
if args.out:
    open(args.out, "w").write("\n".join(lines) + "\n")
