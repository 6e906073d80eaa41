"""Timing of the batched closed-loop rollout (ilqr_problem_closed_loop_dev) with HIP events after a warm-up, 5 runs: the cooperative kernels
(k_closed_loop_coop + k_closed_loop_kp, ilqr_planner_amd/csrc/ilqr_closed_loop.hip) against the generic one (k_closed_loop) on C3, C2 and C4
at B = 256 and 4096, S = 16 and 64, with the bytes a call must move (from the shapes) and its fraction of the 8 TB/s HBM roof:
the plan K | d | xbar | ubar once per (instance, step), x0 and w in, cost, X and U out.
Then, per (workload, B), the analytic covariance (ilqr_problem_closed_loop_cov_dev asking for kp_var and lim_z only): the row kernel
k_cl_cov_rows against the generic k_cl_cov, and next to them ilqr_problem_closed_loop_noise_dev asking for `stats` only at S = 64 -- the
sampled answer to the same question.  Both move the plan once, B (T-1) (n_u rowp + n_x + n_u) 8 bytes.
Usage: python scripts/time_closed_loop.py [--reps R] [--only-cov]"""
import argparse
import os
import sys

import numpy as np
import torch

torch.cuda.init()  # torch's device first, then the library's context
sys.path.insert(0, ".")
from ilqr_planner_amd import capi, workloads  # noqa: E402

ROOF = 8e12  # B/s
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only-cov", action="store_true", help="skip the table of the sampled rollout with caller-given x0 and w")
args = ap.parse_args()

ctx = capi.Context(0)
stream = torch.cuda.Stream()  # a stream of its own: the events below must bracket the library's launches (the default stream is handle 0)
ctx.set_stream(stream.cuda_stream)
dev = torch.device("cuda:0")


def timed(fn):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps * 1e3  # us


for name in ("C3", "C2", "C4"):
    cfg = workloads.config(name)
    T = cfg["T"]
    for B in (256, 4096):
        desc, inp = workloads.make_batch(ctx, cfg, B=B)
        p = workloads.load_batch(ctx, desc, inp, B)
        workloads.run_solver(p, cfg, nb_iter=3, early_stop=False)
        ctx.synchronize()
        nx, nu = p.dims.n_x, p.dims.n_u
        xbar0 = torch.as_tensor(p.X()[:, 0], device=dev)
        plan_bytes = B * (T - 1) * (nu * ((nx + 2) & ~1) + nx + nu) * 8
        kp_var = torch.zeros((B, p.n_kp, 5), dtype=torch.float64, device=dev)
        lim_z = torch.zeros((B,), dtype=torch.float64, device=dev)
        stats = torch.zeros((B, 5), dtype=torch.float64, device=dev)
        nz = p.noise(1, 1e-3, 1e-3)
        torch.cuda.synchronize()
        calls = {"cov": lambda: p.closed_loop_cov_dev(1e-3, 1e-3, kp_var_ptr=kp_var.data_ptr(), lim_z_ptr=lim_z.data_ptr()),
                 "noise stats S=64": lambda: p.closed_loop_noise_dev(64, nz, None, False, None, stats.data_ptr())}
        for what, fn in calls.items():
            for variant in ("planned", "generic"):
                if variant == "generic":
                    os.environ["ILQR_HIP_PATH"] = "v1"
                else:
                    os.environ.pop("ILQR_HIP_PATH", None)
                us = timed(fn)
                print(f"{name} T={T} B={B:5d} {what:<16} {variant:<8} {us:10.1f} us  {us / (T - 1):7.2f} us/step  plan {plan_bytes / 1e6:7.1f} MB  "
                      f"{100 * plan_bytes / (us * 1e-6) / ROOF:5.2f} % of roof", flush=True)
            os.environ.pop("ILQR_HIP_PATH", None)
        for S in (() if args.only_cov else (16, 64)):
            gen = torch.Generator(device=dev).manual_seed(S)
            x0 = (xbar0[:, None, :] + 1e-2 * torch.randn((B, S, nx), dtype=torch.float64, device=dev, generator=gen)).contiguous()
            w = 1e-3 * torch.randn((B, S, T - 1, nx), dtype=torch.float64, device=dev, generator=gen)
            cost = torch.zeros((B, S), dtype=torch.float64, device=dev)
            X = torch.zeros((B, S, T, nx), dtype=torch.float64, device=dev)
            U = torch.zeros((B, S, T - 1, nu), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            call = lambda: p.closed_loop_dev(S, x0.data_ptr(), w.data_ptr(), False, cost.data_ptr(), X.data_ptr(), U.data_ptr())  # noqa: E731
            plan_bytes = B * (T - 1) * (nu * ((nx + 2) & ~1) + nx + nu) * 8
            io_bytes = (x0.numel() + w.numel() + cost.numel() + X.numel() + U.numel()) * 8
            res = {}
            for variant in ("cooperative", "generic"):
                if variant == "generic":
                    os.environ["ILQR_HIP_PATH"] = "v1"
                else:
                    os.environ.pop("ILQR_HIP_PATH", None)
                us = timed(call)
                res[variant] = (us, cost.clone(), X.clone())
                nb = plan_bytes + io_bytes
                print(f"{name} T={T} B={B:5d} S={S:3d} {variant:<11} {us:10.1f} us  {us / (T - 1):7.2f} us/step  {nb / 1e6:9.1f} MB "
                      f"(plan {plan_bytes / 1e6:.1f})  {100 * nb / (us * 1e-6) / ROOF:5.1f} % of roof", flush=True)
            os.environ.pop("ILQR_HIP_PATH", None)
            bits = lambda t: t.view(torch.int64)  # noqa: E731  (an execution that diverges is NaN on both sides)
            same = all(torch.equal(bits(res["cooperative"][i]), bits(res["generic"][i])) for i in (1, 2))
            print(f"    cooperative / generic: {res['cooperative'][0] / res['generic'][0]:.2f}; results bit-identical: {same}", flush=True)
            del x0, w, cost, X, U, res
        p.close()
ctx.close()
