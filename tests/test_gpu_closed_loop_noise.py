"""Closed-loop rollouts with noise drawn on the device (ilqr_problem_closed_loop_noise): the cooperative kernels where plan_closed_loop chooses
them and the generic one under the pin, with the generator of ilqr_noise.hpp inside both, and k_closed_loop_stats -- held to the checks of
tests/closed_loop_noise.py: the draw is the definition (1), the rollout is the existing one (2), cooperative = generic bit for bit (3), cut-outs
(4), statistics (5), the stream (6), a call beyond the 32-bit reach of the per-step arrays (7), the interfaces (8).  B = 13;
S = 1, 3, 4, 5, 16, 17, 64, 65 over T = 2, 3, 9 and depth + 1 of the staged block (the scheme of tests/test_gpu_closed_loop.py).  The host build
of the generic kernel: tests/test_closed_loop_noise_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads
from tests import closed_loop as cl
from tests import closed_loop_noise as cn
from tests import test_gpu_closed_loop as base
from tests.helpers import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

SHAPES = cn.SHAPES + ("shared", "limits")


def combos(name):
    """[(T, samples)]: T = 2 (only the start draw and step 0), 3 and 9 on a few sample counts, and depth + 1 on every S that reaches the depth."""
    kind, nd = cl.SYSTEM[name]
    by_T = {2: {1, 4}, 3: {3, 5}, 9: {5, 17}}
    for S in base.S_ALL:
        d = base.staged_depth(kind, nd, S)
        by_T.setdefault(9 if d is None else d + 1, set()).add(S)
    return [(T, tuple(sorted(s))) for T, s in sorted(by_T.items())]


@pytest.fixture(scope="module")
def ctx():
    import torch

    torch.cuda.init()  # torch's device first, then the library's context (the device-pointer test hands torch tensors to the library)
    c = capi.Context(0)
    yield c
    c.close()


def test_combos_cover_every_sample_count():
    for name in SHAPES:
        cs = combos(name)
        assert {s for _, ss_ in cs for s in ss_} == set(base.S_ALL), name
        assert {2, 3, 9} <= {T for T, _ in cs} and max(T for T, _ in cs) <= 9


@pytest.mark.parametrize("name", SHAPES)
def test_draw_rollout_statistics_and_generic_kernel(ctx, name):
    worst = dict(dev=0.0)
    for T, samples in combos(name):
        print(cn.check_case(ctx, name, T, samples, worst=worst, compare_generic=True), flush=True)


@pytest.mark.parametrize("name", ["C2", "C3", "C4t1"])
def test_cut_out_with_offsets_reproduces_the_large_call(ctx, name):
    cn.check_cut_out(ctx, name)
    with cl.generic_pin():
        cn.check_cut_out(ctx, name)


def test_stream_is_sound(ctx):
    for zs in cn.check_stream_of_call(ctx):
        print(", ".join(f"{k} {v:.2f}" for k, v in zs.items()))


def test_reach_beyond_the_32_bit_offsets_of_the_per_step_arrays(ctx):
    """(7): C2 at T = 400, B = 13, S = 59 000: B S T n_x > 2^31; cost and stats only"""
    T, S = 400, 59000
    cfg, desc, inp, _ = cl.make_case(ctx, "C2", T)
    p = cl.solve(ctx, cfg, desc, inp)
    try:
        nx = p.dims.n_x
        assert cl.B * S * T * nx > 2 ** 31
        sw, sx = np.full(nx, 1e-3), np.full(nx, 1e-2)
        whole = p.closed_loop_noise(S, 7, sw, sx)
        assert np.all(np.isfinite(whole.cost))
        cn.check_stats(whole.stats, whole.cost, "reach")
        for off in (0, S // 2):
            half = p.closed_loop_noise(S // 2, 7, sw, sx, sample_offset=off)
            assert np.array_equal(half.cost, whole.cost[:, off:off + S // 2]), f"samples {off} .. differ from the whole call"
        one = np.zeros(1)
        dp = C.POINTER(C.c_double)
        nz = p.noise(7, sw, sx)
        cl._refused(lambda: ctx.check(p.L.ilqr_problem_closed_loop_noise(p.h, S, C.byref(nz), None, 0, one.ctypes.data_as(dp), None, one.ctypes.data_as(dp),
                                                                         None, None)), "32-bit offsets")
    finally:
        p.close()


def _torch_call(p, S, nz, x0, ff):
    import torch

    dev = torch.device("cuda:0")
    x0d = torch.as_tensor(np.ascontiguousarray(x0), device=dev) if x0 is not None else None
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)  # noqa: E731
    cost, stats, stats_only = z(p.B, S), z(p.B, 5), z(p.B, 5)
    X, U, w = z(p.B, S, p.T, p.dims.n_x), z(p.B, S, p.T - 1, p.dims.n_u), z(p.B, S, p.T - 1, p.dims.n_x)
    torch.cuda.synchronize()
    x0p = x0d.data_ptr() if x0d is not None else None
    p.closed_loop_noise_dev(S, nz, x0p, ff, cost.data_ptr(), stats.data_ptr(), X.data_ptr(), U.data_ptr(), w.data_ptr())
    p.closed_loop_noise_dev(S, nz, x0p, ff, None, stats_only.data_ptr())   # the costs stay in the problem's workspace
    p.ctx.synchronize()
    assert torch.equal(stats, stats_only)
    return tuple(t.cpu().numpy() for t in (cost, stats, X, U, w))


def test_error_texts_and_device_pointers(ctx):
    cn.check_interfaces(ctx, _torch_call)


def test_pylqr_closed_loop_batch_with_seed_equals_the_c_abi(ctx):
    sys.path.insert(0, os.path.join(ROOT, "ilqr_planner_amd", "pylqr"))
    from PyLQR.sim import KDLRobot
    from PyLQR.solver import AL_ILQR, Constraint, ILQRRecursive
    from PyLQR.system import PosOrnKeypoint, PosOrnPlannerSys

    T, S, Bn = 9, 5, cl.B
    for name in ("C2", "C3"):
        cfg, desc, inp, _ = cl.make_case(ctx, name, T)
        p = cl.solve(ctx, cfg, desc, inp)
        try:
            plan = cl.plan_of(p)
            sw, sx = cn.sigma_vectors(7, *cn.scales(name))
            centre = plan["X"][:, None, 0, :] + 0.01 * np.arange(S)[None, :, None]
            want = p.closed_loop_noise(S, 77, sw, sx, x0=centre, with_feedforward=True, want_X=True, want_U=True)
            x0, w = cl.perturbations(plan, S, seed=3)
            old = p.closed_loop(x0, w, with_feedforward=True)
        finally:
            p.close()
        q0 = inp["q0"]
        qMax = np.full(7, 10 * np.pi)
        rbt = KDLRobot(os.path.join(GOLDEN, "panda_chain.urdf"), "panda_link0", "panda_tip", list(q0[0]), [0.0] * 7)
        kps = [PosOrnKeypoint(np.array(tg[0][0:3]), np.array(tg[0][3:7]), np.diag(cfg["Qdiag"][k]), int(inp["kp_t"][k])) for k, tg in enumerate(inp["targets"])]
        sys_ = PosOrnPlannerSys(rbt, kps, list(workloads.control_weights(cfg, 7)), qMax, -qMax, T, 1, cfg["dt"])
        if name == "C2":
            solver, pre = ILQRRecursive(sys_), (inp["U0"], cl.NIT, True, True)
        else:
            al = cfg["al"]
            cons = []
            for _ in range(T - 1):
                c = Constraint()
                c.A, c.b = inp["A"], inp["b"]
                cons.append(c)
            solver = AL_ILQR(sys_, cons, [inp["lambda0"][0, k] for k in range(T - 1)])
            pre = (inp["U0"], cl.NIT, al["lag"], al["penalty"], al["scaling"], True, True)
        common = dict(q0=q0, kp_targets=list(inp["targets"]), with_feedforward=True)
        _, loop = solver.closed_loop_batch(*pre, x0=centre, seed=77, sigma_w=sw, sigma_x0=sx, **common)
        assert loop.stats.shape == (Bn, 5)
        for f, a, b in zip(("cost", "stats", "X", "U"), want[:4], (loop.cost, loop.stats, loop.X, loop.U)):
            assert np.array_equal(a, b), f"{name}: {f}"
        with pytest.raises(RuntimeError, match="either w or seed"):
            solver.closed_loop_batch(*pre, x0=x0, w=w, seed=1, **common)
        _, loop = solver.closed_loop_batch(*pre, x0=x0, w=w, **common)   # without the new arguments: today's call, with stats filled
        for a, b in zip(old, (loop.cost, loop.X, loop.U)):
            assert np.array_equal(a, b), name
        cn.check_stats(loop.stats, loop.cost, f"{name} PyLQR stats of the caller's w", need_spread=0)
