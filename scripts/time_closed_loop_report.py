"""Timing of the closed-loop report with HIP events around synchronised calls, after a warm-up per shape, on C3 and C4 at B = 256 and 4096,
S = 16 and 64:
 (a) ilqr_problem_closed_loop_noise_dev with only `stats` (the existing entry point);
 (b) ilqr_problem_closed_loop_report_dev with only kp_stats + outcome (kp_err and lim_cost stay in the problem's workspace);
 (c) ilqr_problem_closed_loop_report_dev with every output.
(b) - (a) is what the report adds: k_closed_loop_kp_err (a second FK pass over the keypoint states), the two reductions and the rollout's stores.

  python scripts/time_closed_loop_report.py [--reps R]
  python scripts/time_closed_loop_report.py --ab OLD.so NEW.so     (a) alone on two builds of the library, alternating OLD NEW OLD NEW OLD, each in
                                                                   a process of its own; the OLD runs among themselves give the spread
  python scripts/time_closed_loop_report.py --one                  C3, B = 4096, S = 64, (c) only: the run to put under
                                                                   rocprofv3 --kernel-trace --stats for the per-kernel split
Experiment tooling; nothing in the product reads a library path from the command line."""
import argparse
import ctypes
import os
import subprocess
import sys
import types

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--ab", nargs=2, metavar=("OLD", "NEW"))
ap.add_argument("--lib", help="time (a) alone on this build (it may predate the report)")
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
    for k in rows[0][1]:
        old = [r[k] for t, r in rows if t == "old"]
        new = [r[k] for t, r in rows if t == "new"]
        print(f"{k}: old {min(old):9.1f} .. {max(old):9.1f} us (spread {100 * (max(old) - min(old)) / min(old):4.1f} %)   new {min(new):9.1f} .. {max(new):9.1f} us   "
              f"new within the spread of old: {min(new) <= max(old)}", flush=True)
    sys.exit(0)

import torch  # noqa: E402

torch.cuda.init()  # torch's device first, then the library's context
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ilqr_planner_amd import capi  # noqa: E402

if args.lib:
    capi.LIB_PATH = args.lib
    lib = ctypes.CDLL(args.lib)
    for sym in ("ilqr_problem_closed_loop_report", "ilqr_problem_closed_loop_report_dev"):
        if not hasattr(lib, sym):   # a build from before the report: capi.load() declares the prototypes of symbols it does not have
            setattr(lib, sym, types.SimpleNamespace())
    ctypes.CDLL = lambda path, *a, **k: lib
from ilqr_planner_amd import workloads  # noqa: E402

ctx = capi.Context(0)
stream = torch.cuda.Stream()  # a stream of its own: the events below must bracket the library's launches
ctx.set_stream(stream.cuda_stream)
dev = torch.device("cuda:0")
SW, SX0 = 1e-3, 1e-2


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
        workloads.run_solver(p, cfg, nb_iter=3, early_stop=False)
        ctx.synchronize()
        nz = p.noise(1, SW, SX0)
        for S in (64,) if args.one else (16, 64):
            stats = z(B, 5)
            a_us = None
            if not args.one:
                a_us = timed(lambda: p.closed_loop_noise_dev(S, nz, None, False, None, stats.data_ptr()))
            if args.lib:
                print(f"AB {name}/B{B}/S{S} {a_us:.1f}", flush=True)
                continue
            tol = p.tol([0.02, 0.1, -1, -1, -1], 0.0)
            cost, kp_err, kp_stats, lim_cost, outcome = z(B, S), z(B, S, p.n_kp, 5), z(B, p.n_kp, 12), z(B, S), z(B, 4)
            torch.cuda.synchronize()
            c_us = timed(lambda: p.closed_loop_report_dev(S, nz, None, None, False, tol, cost.data_ptr(), stats.data_ptr(), kp_err.data_ptr(),
                                                          kp_stats.data_ptr(), lim_cost.data_ptr(), outcome.data_ptr()))
            if args.one:
                print(f"{name} T={cfg['T']} B={B} S={S}  (c) report, every output {c_us:10.1f} us", flush=True)
                continue
            b_us = timed(lambda: p.closed_loop_report_dev(S, nz, None, None, False, tol, None, None, None, kp_stats.data_ptr(), None, outcome.data_ptr()))
            print(f"{name} T={cfg['T']} B={B:5d} S={S:3d}  (a) closed_loop_noise_dev, stats only {a_us:10.1f} us   (b) report, kp_stats + outcome {b_us:10.1f} us   "
                  f"(c) report, every output {c_us:10.1f} us   (b)/(a) {b_us / a_us:5.2f}   n_ok / (B S) {outcome[:, 0].sum().item() / (B * S):.3f}", flush=True)
        p.close()
ctx.close()
