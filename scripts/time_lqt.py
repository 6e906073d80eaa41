"""Timing of the batched LQT path (ilqr_planner_amd/csrc/ilqr_lqt.hip) with HIP events after warm-up, per call of the C ABI, with the bytes
each call moves (from the shapes) and its fraction of the 8 TB/s HBM roof.
  solve_dp B=1   shared Qs: k_lqt_chain (one wave) + k_lqt_affine for one instance -- the two latency chains of the DP form
  solve_dp       shared Qs at B: k_lqt_chain + k_lqt_affine
  rollout        solve_lin_al after solve_dp: k_lqt_rollout alone
  per-instance   solve_dp with per-instance Qs: k_lqt_chain<fused>, one wave per instance
The split of solve_dp between its two kernels comes from a kernel trace (rocprofv3 --kernel-trace --stats -- python scripts/time_lqt.py).
Usage: python scripts/time_lqt.py [--reps R]"""
import argparse
import sys

import numpy as np
import torch

torch.cuda.init()  # torch's device first, then the library's context
sys.path.insert(0, ".")
from ilqr_planner_amd import capi  # noqa: E402

ROOF = 8e12  # B/s
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()

ctx = capi.Context(0)
stream = torch.cuda.Stream()  # a stream of its own: the events below must bracket the library's launches (the default stream is handle 0)
ctx.set_stream(stream.cuda_stream)


def timed(fn):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(args.reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps * 1e3  # us


def problem(n, m, N, B, per):
    rng = np.random.default_rng(0)
    A = np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n)
    Bm = rng.standard_normal((n, m)) / np.sqrt(n)
    G = rng.standard_normal((N, n, n))
    Qs = G @ G.transpose(0, 2, 1) / n + 0.5 * np.eye(n)
    if per:
        Qs = np.broadcast_to(Qs, (B,) + Qs.shape)
    return A, Bm, Qs, rng.standard_normal((B, N, n))


def line(name, us, nbytes, note=""):
    frac = nbytes / (us * 1e-6) / ROOF if nbytes else 0.0
    print(f"  {name:<9} {us:10.1f} us  {nbytes / 1e6:9.1f} MB  {100 * frac:5.1f} % of roof  {note}", flush=True)


N = 200
for n, m in ((14, 7), (4, 2)):
    B = 4096
    print(f"n={n} m={m} N={N} B={B} shared Qs", flush=True)
    A, Bm, Qs, mu = problem(n, m, N, 1, False)
    one = capi.LQTBatch(ctx, A, Bm, Qs, mu, 0.1)
    t_one = timed(one.solve_dp)
    one.close()
    A, Bm, Qs, mu = problem(n, m, N, B, False)
    lq = capi.LQTBatch(ctx, A, Bm, Qs, mu, 0.1)
    t_dp = timed(lq.solve_dp)
    t_roll = timed(lq.solve_lin_al)
    lq.close()
    line("dp B=1", t_one, 0, f"{t_one / (N - 1):.2f} us/step (chain + affine of one instance: latency)")
    line("solve_dp", t_dp, B * N * n * 16, "mu in, d out")
    line("rollout", t_roll, B * N * (3 * n + m) * 8, "mu, d in; X, U out")
    B = 1024
    print(f"n={n} m={m} N={N} B={B} per-instance Qs", flush=True)
    A, Bm, Qs, mu = problem(n, m, N, B, True)
    lq = capi.LQTBatch(ctx, A, Bm, Qs, mu, 0.1, qs_per_instance=True)
    t_pi = timed(lq.solve_dp)
    t_roll = timed(lq.solve_lin_al)
    lq.close()
    line("solve_dp", t_pi, B * N * (2 * n * n + 2 * m * n + 2 * n) * 8, f"{t_pi / (N - 1):.2f} us/step, one wave per instance (Q, mu in; P, L, H, d out)")
    line("rollout", t_roll, B * N * (3 * n + m) * 8)
ctx.close()
