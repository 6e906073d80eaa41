"""Batched closed-loop rollouts of the tracking law on the device (ilqr_problem_closed_loop): the cooperative kernels k_closed_loop_coop +
k_closed_loop_kp where plan_closed_loop chooses them, and the generic k_closed_loop under the pin, held to the checks of tests/closed_loop.py --
the NumPy replay of the law with the oracle's step and cost ((a), (b)), the definition through ilqr_problem_track (c), the null case (d) -- and
to each other bit for bit (e).  B = 13; S = 1, 3, 4, 5, 16, 17, 64, 65 cross every lane-group boundary and the padding of a partial group; the
horizons are T = 2, 3, 25 and, for every depth d of the staged block that the shape's samples reach, d - 1, d, d + 1 and 2 d + 1.  Then batch
independence (f) and the interfaces (g).  The host build of the generic kernel: tests/test_closed_loop_cpu.py."""
import os
import sys

import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads
from tests import closed_loop as cl
from tests.helpers import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

S_ALL = (1, 3, 4, 5, 16, 17, 64, 65)
LDS_BUDGET, MAX_DEPTH = 40 * 1024, 8   # ilqr_closed_loop_plan.hpp (its table: tests/cpp/closed_loop_plan_main.cpp)


def staged_depth(kind, nd, S):
    """depth of plan_closed_loop for S samples of system (kind, nd), or None where it returns the generic kernel"""
    if S < 4:
        return None
    tm = 1 if kind in (1, 3) else 0
    nx, nu = (1 if kind in (2, 3) else nd) * 7 + tm, 7 + tm
    stride = (nu * ((nx + 2) & ~1) + nx + nu) | 1
    ns = 4
    while ns < S and ns < 64:
        ns *= 2
    return min(MAX_DEPTH, LDS_BUDGET // ((64 // ns) * stride * 8))


def combos(name):
    """[(T, samples)]: T = 2, 3, 25 on a few sample counts; around every depth d the shape reaches, d - 1 and d on the smallest S of that depth,
    d + 1 on all of them (every group boundary), 2 d + 1 on the smallest and the largest."""
    kind, nd = cl.SYSTEM[name]
    by_T = {2: {1, 4}, 3: {3, 5}, 25: {5, 16}}
    depths = {}
    for S in S_ALL:
        d = staged_depth(kind, nd, S)
        if d is not None:
            depths.setdefault(d, []).append(S)
    for d, Sd in depths.items():
        for T, samples in ((d - 1, Sd[:1]), (d, Sd[:1]), (d + 1, Sd), (2 * d + 1, [Sd[0], Sd[-1]])):
            if T >= 2:
                by_T.setdefault(T, set()).update(samples)
    return [(T, tuple(sorted(s))) for T, s in sorted(by_T.items())]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def test_combos_cover_every_sample_count_and_depth():
    for name in cl.SHAPES + cl.EXTRA:
        cs = combos(name)
        assert {s for _, ss_ in cs for s in ss_} == set(S_ALL), name
        assert {2, 3, 25} <= {T for T, _ in cs}


@pytest.mark.parametrize("name", cl.SHAPES + cl.EXTRA)
def test_closed_loop_against_replay_and_generic_kernel(ctx, name):
    stats = cl.new_stats()
    for T, samples in combos(name):
        print(cl.check_case(ctx, name, T, samples, stats=stats, compare_generic=True), flush=True)
    print(f"{name}: {stats['n']} samples, {stats['ill']} ill-conditioned (worst ratio {stats['worst_ratio']:.2f} of {cl.ILL_FACTOR:g}); worst deviation "
          f"of the others: X {stats['worst_X']:.3e}, U {stats['worst_U']:.3e}, J {stats['worst_J']:.3e} relative")


@pytest.mark.parametrize("name,kp", [("C2", (0, 8)), ("C2", (5, 6)), ("C4t1", (0, 8)), ("C2nd", (2, 3))])
def test_keypoints_at_step_0_at_the_last_step_and_two_in_one_block(ctx, name, kp):
    """T = 9: a keypoint at step 0 and one at the last step, or two inside one staged block"""
    print(cl.check_case(ctx, name, 9, (5, 17), kp=kp, compare_generic=True))


def _cut(inp, bs):
    out = dict(inp)
    for k in ("q0", "dq0", "U0", "lambda0"):
        if k in inp:
            out[k] = np.ascontiguousarray(inp[k][bs])
    out["targets"] = [np.ascontiguousarray(t[bs]) for t in inp["targets"]]
    return out


@pytest.mark.parametrize("name", ["C2", "C3", "C4t1"])
def test_cut_out_of_batch_and_samples_reproduces_the_large_call(ctx, name):
    """(f): instances 2 .. 10 and samples 1 .. 13 of a 13 x 17 call, as a call of their own"""
    T, S = 9, 17
    cfg, desc, inp, _ = cl.make_case(ctx, name, T)
    p = cl.solve(ctx, cfg, desc, inp)
    try:
        x0, w = cl.perturbations(cl.plan_of(p), S, seed=7)
        big = p.closed_loop(x0, w, with_feedforward=True)
    finally:
        p.close()
    bs, ss_ = slice(2, 11), slice(1, 14)
    q = cl.solve(ctx, cfg, desc, _cut(inp, bs))
    try:
        small = q.closed_loop(x0[bs, ss_], w[bs, ss_], with_feedforward=True)
    finally:
        q.close()
    for a, b in zip(big, small):
        assert np.array_equal(a[bs, ss_], b)


def _torch_call(p, S, x0, w, ff):
    import torch

    dev = torch.device("cuda:0")
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev) if a is not None else None  # noqa: E731
    x0d, wd = t(x0), t(w)
    cost = torch.zeros((p.B, S), dtype=torch.float64, device=dev)
    X = torch.zeros((p.B, S, p.T, p.dims.n_x), dtype=torch.float64, device=dev)
    U = torch.zeros((p.B, S, p.T - 1, p.dims.n_u), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    p.closed_loop_dev(S, x0d.data_ptr() if x0d is not None else None, wd.data_ptr() if wd is not None else None, ff, cost.data_ptr(), X.data_ptr(),
                      U.data_ptr())
    p.ctx.synchronize()
    return cost.cpu().numpy(), X.cpu().numpy(), U.cpu().numpy()


def test_error_texts_and_device_pointers(ctx):
    cl.check_interfaces(ctx, _torch_call, batch_solver=True)


def test_pylqr_closed_loop_batch_equals_the_c_abi(ctx):
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
            x0, w = cl.perturbations(plan, S, seed=3)
            want = p.closed_loop(x0, w, with_feedforward=True)
        finally:
            p.close()
        q0 = inp["q0"]
        qMax = np.full(7, 10 * np.pi)
        rbt = KDLRobot(os.path.join(GOLDEN, "panda_chain.urdf"), "panda_link0", "panda_tip", list(q0[0]), [0.0] * 7)
        kps = [PosOrnKeypoint(np.array(tg[0][0:3]), np.array(tg[0][3:7]), np.diag(cfg["Qdiag"][k]), int(inp["kp_t"][k])) for k, tg in enumerate(inp["targets"])]
        sys_ = PosOrnPlannerSys(rbt, kps, list(workloads.control_weights(cfg, 7)), qMax, -qMax, T, 1, cfg["dt"])
        args = dict(q0=q0, kp_targets=list(inp["targets"]), x0=x0, w=w, with_feedforward=True)
        if name == "C2":
            res, loop = ILQRRecursive(sys_).closed_loop_batch(inp["U0"], cl.NIT, True, True, **args)
        else:
            al = cfg["al"]
            cons = []
            for _ in range(T - 1):
                c = Constraint()
                c.A, c.b = inp["A"], inp["b"]
                cons.append(c)
            res, loop = AL_ILQR(sys_, cons, [inp["lambda0"][0, k] for k in range(T - 1)]).closed_loop_batch(
                inp["U0"], cl.NIT, al["lag"], al["penalty"], al["scaling"], True, True, **args)
        assert np.array_equal(res.X, plan["X"]) and np.array_equal(res.U, plan["U"]), f"{name}: the two lowerings solve different problems"
        assert loop.cost.shape == (Bn, S) and loop.X.shape == (Bn, S, T, 7) and loop.U.shape == (Bn, S, T - 1, 7)
        for a, b in zip(want, (loop.cost, loop.X, loop.U)):
            assert np.array_equal(a, b), name
