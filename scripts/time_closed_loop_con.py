"""Timing of the constraint report with HIP events around synchronised calls, after a warm-up per shape, on C3 and C4 at B = 256 and 4096,
S = 16 and 64 (C4 carries no rows of its own: it gets the one row of the AL workloads, q_6 <= 2.0):
 (a) ilqr_problem_closed_loop_report_dev with kp_stats + outcome (the existing entry point);
 (b) ilqr_problem_closed_loop_report_con_dev with the same plus con_stats + outcome_con (con_max and con_steps stay in the problem's workspace);
 (c) ilqr_problem_closed_loop_cov_dev with lim_z;
 (d) ilqr_problem_closed_loop_cov_con_dev with lim_z + con_z.
(b) - (a) is what the rows add to a rollout: cl_con at every step, two stores per execution and the two reductions.

  python scripts/time_closed_loop_con.py [--reps R]
  python scripts/time_closed_loop_con.py --ab OLD.so NEW.so     the existing calls alone -- (a), closed_loop_noise_dev with only `stats`, (c) -- on two
                                                                builds of the library, alternating OLD NEW OLD NEW OLD, each in a process of its own;
                                                                the OLD runs among themselves give the spread
  python scripts/time_closed_loop_con.py --one                  C3, B = 4096, S = 64, (b) only: the run to put under
                                                                rocprofv3 --kernel-trace --stats for the per-kernel split
Experiment tooling; nothing in the product reads a library path from the command line."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import types

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--ab", nargs=2, metavar=("OLD", "NEW"))
ap.add_argument("--lib", help="time the existing calls alone on this build (it may predate the constraint report)")
ap.add_argument("--one", action="store_true")
args = ap.parse_args()

if args.ab:
    rows = []
    for tag, lib in zip(("old", "new", "old", "new", "old"), (args.ab * 3)[:5]):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--lib", os.path.abspath(lib)], capture_output=True, text=True)
        vals = [l for l in out.stdout.splitlines() if l.startswith("AB ")]
        if out.returncode or not vals:
            print(tag, "FAILED", out.stderr[-1500:], flush=True)
            sys.exit(1)
        rows.append((tag, dict((v.split()[1], float(v.split()[2])) for v in vals)))
        print(f"{tag:4s}", "  ".join(f"{k} {v:9.1f}" for k, v in rows[-1][1].items()), flush=True)
    worst = {"rollout": 0.0, "cov": 0.0}   # the rollout calls (report, noise) and the covariance call, each against its own spread
    for k in rows[0][1]:
        old = [r[k] for t, r in rows if t == "old"]
        new = [r[k] for t, r in rows if t == "new"]
        mo, mn = statistics.median(old), statistics.median(new)
        kind = "cov" if k.endswith("/cov") else "rollout"
        worst[kind] = max(worst[kind], mn / mo - 1)
        print(f"{k}: old {min(old):9.1f} .. {max(old):9.1f} us (spread {100 * (max(old) - min(old)) / min(old):4.1f} %, median {mo:9.1f})   "
              f"new {min(new):9.1f} .. {max(new):9.1f} us (median {mn:9.1f})   new / old {100 * (mn / mo - 1):+5.2f} %", flush=True)
    for kind, w in worst.items():
        print(f"largest new / old of the medians, {kind} calls: {100 * w:+.2f} %  (within 2 %: {w <= 0.02})", flush=True)
    sys.exit(0)

import torch  # noqa: E402

torch.cuda.init()  # torch's device first, then the library's context
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ilqr_planner_amd import capi  # noqa: E402

if args.lib:
    capi.LIB_PATH = args.lib
    lib = ctypes.CDLL(args.lib)
    for sym in capi.EXPORTS:
        if not hasattr(lib, sym):   # a build from before the constraint report: capi.load() declares the prototypes of symbols it does not have
            setattr(lib, sym, types.SimpleNamespace())
    ctypes.CDLL = lambda path, *a, **k: lib
import numpy as np  # noqa: E402

from ilqr_planner_amd import workloads  # noqa: E402

ctx = capi.Context(0)
stream = torch.cuda.Stream()  # a stream of its own: the events below must bracket the library's launches
ctx.set_stream(stream.cuda_stream)
dev = torch.device("cuda:0")
SW, SX0, CON_TOL = 1e-3, 1e-2, 0.0


def timed(fn):
    with torch.cuda.stream(stream):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            fn()
        e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps * 1e3  # us


z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)  # noqa: E731
for name in ("C3",) if args.one else ("C3", "C4"):
    cfg = workloads.config(name)
    for B in (4096,) if args.one else (256, 4096):
        desc, inp = workloads.make_batch(ctx, cfg, B=B)
        p = workloads.load_batch(ctx, desc, inp, B)
        if "A" not in inp:   # the row of the AL workloads; the unconstrained solver does not look at it
            A = np.zeros((1, p.dims.n_x + p.dims.n_u))
            A[0, 5] = 1.0
            p.set_constraints(A, np.array([2.0]))
        workloads.run_solver(p, cfg, nb_iter=3, early_stop=False)
        ctx.synchronize()
        nz = p.noise(1, SW, SX0)
        tol = p.tol([0.02, 0.1, -1, -1, -1], 0.0)
        lim_z = z(B)
        c_us = None if args.one else timed(lambda: p.closed_loop_cov_dev(SW, SX0, lim_z_ptr=lim_z.data_ptr()))
        if args.lib:
            print(f"AB {name}/B{B}/cov {c_us:.1f}", flush=True)
        elif not args.one:
            con_z = z(B)
            d_us = timed(lambda: p.closed_loop_cov_con_dev(SW, SX0, lim_z_ptr=lim_z.data_ptr(), con_z_ptr=con_z.data_ptr()))
            print(f"{name} T={cfg['T']} B={B:5d}         (c) closed_loop_cov_dev, lim_z {c_us:10.1f} us   (d) cov_con, lim_z + con_z {d_us:10.1f} us   "
                  f"(d)/(c) {d_us / c_us:5.2f}   finite con_z {int(torch.isfinite(con_z).sum().item())} of {B}", flush=True)
        for S in (64,) if args.one else (16, 64):
            stats, kp_stats, outcome = z(B, 5), z(B, p.n_kp, 12), z(B, 4)
            con_stats, outcome_con = z(B, 6), z(B, 5)
            report = lambda: p.closed_loop_report_dev(S, nz, None, None, False, tol, None, None, None, kp_stats.data_ptr(), None, outcome.data_ptr())  # noqa: E731
            report_con = lambda: p.closed_loop_report_con_dev(S, nz, None, None, False, tol, CON_TOL, kp_stats_ptr=kp_stats.data_ptr(),  # noqa: E731
                                                              outcome_ptr=outcome.data_ptr(), con_stats_ptr=con_stats.data_ptr(),
                                                              outcome_con_ptr=outcome_con.data_ptr())
            if args.one:
                print(f"{name} T={cfg['T']} B={B} S={S}  (b) report_con, reductions only {timed(report_con):10.1f} us", flush=True)
                continue
            a_us = timed(report)
            if args.lib:
                n_us = timed(lambda: p.closed_loop_noise_dev(S, nz, None, False, None, stats.data_ptr()))
                print(f"AB {name}/B{B}/S{S}/report {a_us:.1f}", flush=True)
                print(f"AB {name}/B{B}/S{S}/noise {n_us:.1f}", flush=True)
                continue
            b_us = timed(report_con)
            print(f"{name} T={cfg['T']} B={B:5d} S={S:3d}  (a) report, kp_stats + outcome {a_us:10.1f} us   (b) report_con, + con_stats + outcome_con {b_us:10.1f} us   "
                  f"(b)/(a) {b_us / a_us:5.2f}   n_ok / (B S) {outcome[:, 0].sum().item() / (B * S):.3f} -> {outcome_con[:, 0].sum().item() / (B * S):.3f} with the rows", flush=True)
        p.close()
ctx.close()
