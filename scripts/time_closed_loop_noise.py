"""Timing of Monte-Carlo closed-loop statistics with HIP events after a warm-up, 5 runs, on C3 and C4 at B = 256 and 4096, S = 16 and 64:
 (a) with the caller's noise: torch.randn of x0 and w on the device, ilqr_problem_closed_loop_dev with cost only, and a torch reduction of cost
     (mean, variance, min, max, count of non-finite), timed together;
 (b) ilqr_problem_closed_loop_noise_dev with only `stats`: the draws inside the rollout kernels, k_closed_loop_stats for the reduction.
The share of (b) spent in k_closed_loop_stats is the stats launch timed alone on the costs of (b) (the difference of the call with stats and
cost against the call with cost only).  Last line: C3 at B = 4096, S = 512, which (a) cannot run (B S T n_x >= 2^31).
Usage: python scripts/time_closed_loop_noise.py [--reps R]"""
import argparse
import sys

import torch

torch.cuda.init()  # torch's device first, then the library's context
sys.path.insert(0, ".")
from ilqr_planner_amd import capi, workloads  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

ctx = capi.Context(0)
stream = torch.cuda.Stream()  # a stream of its own: the events below must bracket the library's launches and torch's
ctx.set_stream(stream.cuda_stream)
dev = torch.device("cuda:0")
SW, SX0 = 1e-3, 1e-2


def timed(fn):
    with torch.cuda.stream(stream):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            fn()
        e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps * 1e3  # us


def noise_us(p, S, nz):
    stats = torch.zeros((p.B, 5), dtype=torch.float64, device=dev)
    cost = torch.zeros((p.B, S), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    both = timed(lambda: p.closed_loop_noise_dev(S, nz, None, False, cost.data_ptr(), stats.data_ptr()))
    roll = timed(lambda: p.closed_loop_noise_dev(S, nz, None, False, cost.data_ptr(), None))
    only = timed(lambda: p.closed_loop_noise_dev(S, nz, None, False, None, stats.data_ptr()))
    return only, max(both - roll, 0.0), stats


for name in ("C3", "C4"):
    cfg = workloads.config(name)
    T = cfg["T"]
    for B in (256, 4096):
        desc, inp = workloads.make_batch(ctx, cfg, B=B)
        p = workloads.load_batch(ctx, desc, inp, B)
        workloads.run_solver(p, cfg, nb_iter=3, early_stop=False)
        ctx.synchronize()
        nx = p.dims.n_x
        xbar0 = torch.as_tensor(p.X()[:, 0], device=dev)
        nz = p.noise(1, SW, SX0)
        for S in (16, 64):
            cost = torch.zeros((B, S), dtype=torch.float64, device=dev)
            out = {}

            def caller_noise():
                x0 = xbar0[:, None, :] + SX0 * torch.randn((B, S, nx), dtype=torch.float64, device=dev)
                w = SW * torch.randn((B, S, T - 1, nx), dtype=torch.float64, device=dev)
                p.closed_loop_dev(S, x0.data_ptr(), w.data_ptr(), False, cost.data_ptr(), None, None)
                fin = torch.isfinite(cost)
                c = torch.where(fin, cost, torch.zeros_like(cost))
                n = fin.sum(1)
                mean = c.sum(1) / n
                var = (torch.where(fin, cost - mean[:, None], torch.zeros_like(cost)) ** 2).sum(1) / (n - 1)
                out["stats"] = torch.stack((mean, var, torch.where(fin, cost, torch.full_like(cost, float("inf"))).amin(1),
                                            torch.where(fin, cost, torch.full_like(cost, float("-inf"))).amax(1), (S - n).double()), 1)

            a_us = timed(caller_noise)
            b_us, st_us, stats = noise_us(p, S, nz)
            print(f"{name} T={T} B={B:5d} S={S:3d}  (a) randn + closed_loop_dev + torch reduction {a_us:10.1f} us   (b) closed_loop_noise_dev, stats only "
                  f"{b_us:10.1f} us   (b)/(a) {b_us / a_us:5.2f}   k_closed_loop_stats {st_us:7.1f} us = {100 * st_us / b_us:4.1f} % of (b)   "
                  f"noise arrays of (a) {(B * S * T * nx) * 8 / 1e6:8.1f} MB   mean of means (a) {out['stats'][:, 0].mean().item():.6g} (b) {stats[:, 0].mean().item():.6g}",
                  flush=True)
            del cost, out
        if name == "C3" and B == 4096:
            S = 512
            assert B * S * T * nx >= 2 ** 31
            b_us, st_us, stats = noise_us(p, S, nz)
            print(f"{name} T={T} B={B:5d} S={S:3d}  (a) cannot run: B S T n_x = {B * S * T * nx} >= 2^31 ({B * S * (T - 1) * nx * 8 / 1e9:.1f} GB of w)   (b) {b_us:10.1f} us   "
                  f"k_closed_loop_stats {st_us:7.1f} us = {100 * st_us / b_us:4.1f} % of (b)   n_bad total {int(stats[:, 4].sum().item())}", flush=True)
        p.close()
ctx.close()
