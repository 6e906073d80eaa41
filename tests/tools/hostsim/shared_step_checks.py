"""Keypoints that share a timestep through the C ABI on the host build of the lane-per-instance kernels (tests/test_shared_steps_cpu.py builds
the library and runs this script in a child process of its own: its library never meets the product library).  The exact reductions of
tests/shared_steps.py against the oracle; the batch solvers' refusal; a decreasing timestep's error text.

    python tests/tools/hostsim/shared_step_checks.py <libilqr_hostsim.so>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ilqr_planner_amd import capi, workloads  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every solve of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import shared_steps as ss  # noqa: E402

B = 3
SHAPES = ("C2", "C3", "C2nd", "C4t1al", "C2h")  # PosOrn 1st order (recursive, AL), 2nd order, PosOrnTime 1st order AL, the hybrid sequence
BATCH_TEXT = "keypoints that share a timestep are not supported by the batch solvers"


def main():
    ctx = capi.Context(0)
    for name in SHAPES:
        for red in ss.REDUCTIONS:
            cfg, desc, inp, cfg_eq, inp_eq = ss.make_case(ctx, name, red, B)
            _, summ = ss.check_against_oracle(ctx, cfg, desc, inp, cfg_eq, inp_eq, f"{name} {red}")
            print(f"{name} {red}: within 1e-4 {summ['frac_within_1e4']:.2f}, proofs {summ['n_proofs']}", flush=True)
    # a plain System with a duplicated step: the kept keypoint against the oracle's last-wins system
    for name in ("C2", "C4t1"):
        cfg, desc, inp, cfg_dup, inp_dup = ss.last_wins_case(ctx, name, B)
        _, summ = ss.check_against_oracle(ctx, cfg, desc, inp, cfg_dup, inp_dup, f"{name} last wins")
        print(f"{name} last wins: within 1e-4 {summ['frac_within_1e4']:.2f}, proofs {summ['n_proofs']}", flush=True)
    # the batch solvers refuse a shared step before they run
    cfg, desc, inp, _, _ = ss.make_case(ctx, "C2", "double", B)
    p = workloads.load_batch(ctx, desc, inp, B)
    psi = workloads.psi_of(dict(kind="unitstep", K=2), cfg["T"], 7)
    for what, call in (("batch_cp", lambda: p.solve_batch_cp(psi, 2)), ("batch", lambda: p.solve_batch(2))):
        try:
            call()
        except RuntimeError as e:
            assert BATCH_TEXT in str(e), (what, str(e))
        else:
            raise AssertionError(f"{what} ran on a shared step")
    assert np.all(p.iters() == 0), "a batch solver ran"
    p.close()
    print("batch solvers refuse a shared step", flush=True)
    # a shared step outside a sequence is refused: a plain System keeps one keypoint per step
    d = ss.rebuild(desc, [dict(src=0), dict(src=1), dict(src=1)])
    d.is_sequence = 0
    try:
        capi.BatchProblem(ctx, d, B)
    except RuntimeError as e:
        assert "unique and ascending unless is_sequence" in str(e), str(e)
    else:
        raise AssertionError("a shared step without is_sequence was accepted")
    # a decreasing timestep is still refused
    d = ss.rebuild(desc, [dict(src=1), dict(src=0)])
    d.kp_timestep[0], d.kp_timestep[1] = cfg["T"] - 1, 3
    try:
        capi.BatchProblem(ctx, d, B)
    except RuntimeError as e:
        assert "non-decreasing" in str(e), str(e)
    else:
        raise AssertionError("decreasing keypoint timesteps were accepted")
    ctx.close()
    print("shared steps: ok")


if __name__ == "__main__":
    main()
