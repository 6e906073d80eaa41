"""Closed-loop rollouts that report keypoint errors and limit violations on the device (ilqr_problem_closed_loop_report): the cooperative
rollout where plan_closed_loop chooses it and the generic one under the pin, both followed by k_closed_loop_kp_err, k_closed_loop_kp_stats and
k_closed_loop_outcome -- held to the checks of tests/closed_loop_report.py: the definition of the errors (1) and of the limit share (2) against
the oracle, the existing results unchanged (3), the reductions (4), the tolerances (5), cooperative = generic bit for bit (6), cut-outs (7), the
plan itself (8), the interfaces (9).  B = 13; S from 1, 4, 5, 17, 65 over T = 2, 3, 9 and depth + 1 of the staged block (the scheme of
tests/test_gpu_closed_loop_noise.py).  The host build of the generic kernel: tests/test_closed_loop_report_cpu.py."""
import os
import sys

import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads
from tests import closed_loop as cl
from tests import closed_loop_noise as cn
from tests import closed_loop_report as cr
from tests import test_gpu_closed_loop as base
from tests.helpers import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

S_ALL = (1, 4, 5, 17, 65)   # 65: a second block of samples behind NS = 64


def combos(name):
    """[(T, samples)]: T = 2, 3 and 9 on a few sample counts, and depth + 1 of the staged block on every S that reaches the depth."""
    kind, nd = cl.SYSTEM["C2" if name in ("C3d", "frame") else name]
    by_T = {2: {1, 4}, 3: {5}, 9: {17}}
    for S in S_ALL:
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
    for name in cr.SHAPES:
        cs = combos(name)
        assert {s for _, ss_ in cs for s in ss_} == set(S_ALL), name
        assert {2, 3, 9} <= {T for T, _ in cs} and max(T for T, _ in cs) <= 9


@pytest.mark.parametrize("name", cr.SHAPES)
def test_report_against_oracle_numpy_and_generic_kernel(ctx, name):
    worst = dict(err=0.0)
    for T, samples in combos(name):
        print(cr.check_case(ctx, name, T, samples, compare_generic=True, worst=worst), flush=True)


@pytest.mark.parametrize("name", ["C2", "C4t1"])
def test_cut_out_with_offsets_reproduces_the_large_call(ctx, name):
    cr.check_cut_out(ctx, name)
    with cl.generic_pin():
        cr.check_cut_out(ctx, name)


def _torch_call(p, S, nz, x0, w, ff, tol, which):
    import torch

    dev = torch.device("cuda:0")
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev) if a is not None else None  # noqa: E731
    x0d, wd = up(x0), up(w)
    shapes = dict(cost=(p.B, S), stats=(p.B, 5), kp_err=(p.B, S, p.n_kp, 5), kp_stats=(p.B, p.n_kp, 12), lim_cost=(p.B, S), outcome=(p.B, 4))
    t = {f: (torch.zeros(shapes[f], dtype=torch.float64, device=dev) if f in which else None) for f in shapes}
    torch.cuda.synchronize()
    ptr = lambda a: a.data_ptr() if a is not None else None  # noqa: E731
    p.closed_loop_report_dev(S, nz, ptr(x0d), ptr(wd), ff, tol, ptr(t["cost"]), ptr(t["stats"]), ptr(t["kp_err"]), ptr(t["kp_stats"]), ptr(t["lim_cost"]),
                             ptr(t["outcome"]))
    p.ctx.synchronize()
    out = {f: (v.cpu().numpy() if v is not None else None) for f, v in t.items()}
    return capi.ClosedLoopReport(out["cost"], out["stats"], out["kp_err"], out["kp_stats"], out["lim_cost"], out["outcome"], None, None, None)


def test_error_texts_device_pointers_and_reductions_only(ctx):
    cr.check_interfaces(ctx, _torch_call)
    with cl.generic_pin():
        cr.check_interfaces(ctx, _torch_call)


def test_pylqr_closed_loop_batch_with_tolerances_equals_the_c_abi(ctx):
    sys.path.insert(0, os.path.join(ROOT, "ilqr_planner_amd", "pylqr"))
    from PyLQR.sim import KDLRobot
    from PyLQR.solver import ILQRRecursive
    from PyLQR.system import PosOrnKeypoint, PosOrnPlannerSys

    T, S, name = 9, 5, "C2"
    cfg, desc, inp, _ = cl.make_case(ctx, name, T)
    p = cl.solve(ctx, cfg, desc, inp)
    try:
        plan = cl.plan_of(p)
        sw, sx = cn.sigma_vectors(7, *cn.scales(name))
        centre = plan["X"][:, None, 0, :] + 0.01 * np.arange(S)[None, :, None]
        kp_tol = [[0.05, 0.2, -1, -1, -1], [0.02, -1, -1, -1, -1]]
        want = p.closed_loop_report(S, 77, sw, sx, x0=centre, with_feedforward=True, kp_tol=kp_tol, lim_tol=0.0, want_X=True, want_U=True)
        x0, w = cl.perturbations(plan, S, seed=3)
        want_w = p.closed_loop_report(x0=x0, w=w, with_feedforward=True, kp_tol=0.03, lim_tol=0.5)
        old = p.closed_loop(x0, w, with_feedforward=True)
    finally:
        p.close()
    q0 = inp["q0"]
    qMax = np.full(7, 10 * np.pi)
    rbt = KDLRobot(os.path.join(GOLDEN, "panda_chain.urdf"), "panda_link0", "panda_tip", list(q0[0]), [0.0] * 7)
    kps = [PosOrnKeypoint(np.array(tg[0][0:3]), np.array(tg[0][3:7]), np.diag(cfg["Qdiag"][k]), int(inp["kp_t"][k])) for k, tg in enumerate(inp["targets"])]
    solver = ILQRRecursive(PosOrnPlannerSys(rbt, kps, list(workloads.control_weights(cfg, 7)), qMax, -qMax, T, 1, cfg["dt"]))
    pre = (inp["U0"], cl.NIT, True, True)
    common = dict(q0=q0, kp_targets=list(inp["targets"]), with_feedforward=True)
    fields = ("cost", "stats", "X", "U", "kp_err", "kp_stats", "lim_cost", "outcome")
    _, loop = solver.closed_loop_batch(*pre, x0=centre, seed=77, sigma_w=sw, sigma_x0=sx, kp_tol=kp_tol, lim_tol=0.0, **common)
    for f in fields:
        assert np.array_equal(getattr(want, f), getattr(loop, f)), f
    _, loop = solver.closed_loop_batch(*pre, x0=x0, w=w, kp_tol=0.03, lim_tol=0.5, **common)
    for f in ("cost", "kp_err", "kp_stats", "lim_cost", "outcome"):
        assert np.array_equal(getattr(want_w, f), getattr(loop, f)), f
    _, loop = solver.closed_loop_batch(*pre, x0=x0, w=w, **common)   # without the new arguments: today's call, no report
    for a, b in zip(old, (loop.cost, loop.X, loop.U)):
        assert np.array_equal(a, b)
    assert loop.kp_err is None and loop.kp_stats is None and loop.lim_cost is None and loop.outcome is None
