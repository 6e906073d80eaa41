"""Closed-loop rollouts with device-drawn noise (ilqr_problem_closed_loop_noise) through the C ABI on the host build of the generic kernel
k_closed_loop and of k_closed_loop_stats (tests/test_closed_loop_noise_cpu.py builds the library and runs this script in a child process of its
own).  C2, C3, C2nd, C4t1, C4, C1j and a 3-joint chain at T = 2, 3, 9 on a ragged batch of 13 with S = 1, 3 and 5, held to the checks (1), (2),
(4), (5), (6) and (8) of tests/closed_loop_noise.py; (3) and (7) need the device.

    python tests/tools/hostsim/closed_loop_noise_checks.py <libilqr_hostsim.so>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

from ilqr_planner_amd import capi  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every call of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import closed_loop_noise as cn  # noqa: E402

HORIZONS = (2, 3, 9)
SAMPLES = (1, 3, 5)


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    worst = dict(dev=0.0)
    for name in cn.SHAPES:
        for T in HORIZONS:
            print(cn.check_case(ctx, name, T, SAMPLES, worst=worst), flush=True)
    for name in ("C2", "C3", "C4t1"):
        cn.check_cut_out(ctx, name)
        print(f"{name}: cut-out ok", flush=True)
    for tag, zs in zip(("restatement", "w_out / sigma"), cn.check_stream_of_call(ctx)):
        print(f"stream of {tag}: " + ", ".join(f"{k} {v:.2f}" for k, v in zs.items()), flush=True)
    cn.check_interfaces(ctx, cn.host_pointer_call)  # on this build a "device" pointer is a host pointer
    print(f"worst deviation of a draw from the restatement: {worst['dev']:.3e} sigma max(1, |z|)", flush=True)
    ctx.close()
    print("closed loop noise: ok")


if __name__ == "__main__":
    main()
