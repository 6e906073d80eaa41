"""Closed-loop executions and their covariance judged against the AL constraint rows on the device (ilqr_problem_closed_loop_report_con,
ilqr_problem_closed_loop_cov_con): the cooperative rollout and the row covariance kernel where the plans choose them, the generic kernels under
the pin, k_closed_loop_con_stats and k_closed_loop_outcome_con -- held to the checks of tests/closed_loop_con.py: the reference (1) with its
precondition (2), the bit equalities (3), the reductions (4), the covariance (5), sampled against analytic (6), the interfaces (7).  B = 13;
T = 2, 3, 9 and 10 (one step past a staged block of depth 8); S from 1 (the generic kernel), 4, 5, 17, 65 (a second wave of samples).  The host
build of the generic kernels: tests/test_closed_loop_con_cpu.py."""
import os
import sys

import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads
from tests import closed_loop as cl
from tests import closed_loop_con as cc
from tests.helpers import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

COMBOS = ((2, (1, 4)), (3, (5,)), (9, (17,)), (10, (5, 65)))


@pytest.fixture(scope="module")
def ctx():
    import torch

    torch.cuda.init()  # torch's device first, then the library's context (the device-pointer test hands torch tensors to the library)
    c = capi.Context(0)
    yield c
    c.close()


def test_combos_cover_every_horizon_and_sample_count():
    assert tuple(T for T, _ in COMBOS) == cc.HORIZONS
    assert {s for _, ss_ in COMBOS for s in ss_} == {1, 4, 5, 17, 65}


@pytest.mark.parametrize("case", list(cc.CASES))
def test_con_against_numpy_report_and_generic_kernel(ctx, case):
    worst = dict(con_max=0.0, con_var=0.0)
    for T, samples in COMBOS:
        print(cc.check_case(ctx, case, T, samples, compare_generic=True, worst=worst), flush=True)


@pytest.mark.parametrize("case", ["C3-m4", "C4t1al-m2-control-per_step"])
def test_cut_out_with_offsets_reproduces_the_large_call(ctx, case):
    cc.check_cut_out(ctx, case)
    with cl.generic_pin():
        cc.check_cut_out(ctx, case)


def test_violated_plan_has_negative_con_z(ctx):
    cc.check_violated_plan(ctx)
    with cl.generic_pin():
        cc.check_violated_plan(ctx)


def test_sample_variance_of_the_rows_against_con_var(ctx):
    print(f"sampled against analytic: {cc.check_sampled_against_analytic(ctx):.3f} of the allowed deviation")


def _torch_call(p, S, nz, x0, ff, tol, con_tol, which):
    import torch

    dev = torch.device("cuda:0")
    x0d = torch.as_tensor(np.ascontiguousarray(x0), device=dev) if x0 is not None else None
    t = {f: (torch.zeros(cc.SHAPES_DEV[f](p, S), dtype=torch.float64, device=dev) if f in which else None) for f in cc.SHAPES_DEV}
    torch.cuda.synchronize()
    p.closed_loop_report_con_dev(S, nz, x0d.data_ptr() if x0d is not None else None, None, ff, tol, con_tol,
                                 **{f + "_ptr": (v.data_ptr() if v is not None else None) for f, v in t.items()})
    p.ctx.synchronize()
    return capi.ClosedLoopReportCon(**{f: (v.cpu().numpy() if v is not None else None) for f, v in t.items()})


def _torch_cov_call(p, sw, sx, which):
    import torch

    dev = torch.device("cuda:0")
    sh = cc.cov_shapes(p)
    t = {f: (torch.zeros(sh[f], dtype=torch.float64, device=dev) if f in which else None) for f in cc.COV_FIELDS}
    torch.cuda.synchronize()
    p.closed_loop_cov_con_dev(sw, sx, **{f + "_ptr": (v.data_ptr() if v is not None else None) for f, v in t.items()})
    p.ctx.synchronize()
    return capi.ClosedLoopCovCon(**{f: (v.cpu().numpy() if v is not None else None) for f, v in t.items()})


def test_error_texts_device_pointers_and_reductions_only(ctx):
    cc.check_interfaces(ctx, _torch_call, _torch_cov_call)
    with cl.generic_pin():
        cc.check_interfaces(ctx, _torch_call, _torch_cov_call)


def test_pylqr_keywords_equal_the_c_abi(ctx):
    sys.path.insert(0, os.path.join(ROOT, "ilqr_planner_amd", "pylqr"))
    from PyLQR.sim import KDLRobot
    from PyLQR.solver import AL_ILQR, Constraint
    from PyLQR.system import PosOrnKeypoint, PosOrnPlannerSys

    T, S, case = 9, 5, "C3-m4"
    cfg, desc, inp = cc.make_case(ctx, case, T)
    al = cfg["al"]
    sw, sx = cc.sigmas_of(case, 7, T)
    kp_tol = [[0.05, 0.2, -1, -1, -1], [0.02, -1, -1, -1, -1]]
    p = workloads.load_batch(ctx, desc, inp, cc.B)
    try:
        p.solve_al(cl.NIT, al["lag"], al["penalty"], al["scaling"], True, True)
        first = p.closed_loop_report_con(0.0, S, 77, sw, sx, with_feedforward=True)
        con_tol = cc.halfway(first.con_max)
        want = p.closed_loop_report_con(con_tol, S, 77, sw, sx, with_feedforward=True, kp_tol=kp_tol, lim_tol=0.0)
        bare = p.closed_loop_report_con(con_tol, S, 77, sw, sx, with_feedforward=True)
        old = p.closed_loop_report(S, 77, sw, sx, with_feedforward=True, kp_tol=kp_tol, lim_tol=0.0, want_X=True, want_U=True)
        cov_old = p.closed_loop_cov(1e-3, 1e-2, want_Sigma=True)
        cov = p.closed_loop_cov_con(1e-3, 1e-2)
    finally:
        p.close()
    q0 = inp["q0"]
    qMax = np.full(7, 10 * np.pi)
    rbt = KDLRobot(os.path.join(GOLDEN, "panda_chain.urdf"), "panda_link0", "panda_tip", list(q0[0]), [0.0] * 7)
    kps = [PosOrnKeypoint(np.array(tg[0][0:3]), np.array(tg[0][3:7]), np.diag(cfg["Qdiag"][k]), int(inp["kp_t"][k])) for k, tg in enumerate(inp["targets"])]
    sys_ = PosOrnPlannerSys(rbt, kps, list(workloads.control_weights(cfg, 7)), qMax, -qMax, T, 1, cfg["dt"])
    cons = []
    for _ in range(T - 1):
        c = Constraint()
        c.A, c.b = inp["A"], inp["b"]
        cons.append(c)
    # a solver per call: AL_ILQR keeps the multipliers of its last solve, as the reference's member does
    make_solver = lambda: AL_ILQR(sys_, cons, [inp["lambda0"][0, k] for k in range(T - 1)])  # noqa: E731
    pre = (inp["U0"], cl.NIT, al["lag"], al["penalty"], al["scaling"], True, True)
    common = dict(q0=q0, kp_targets=list(inp["targets"]))
    loop_kw = dict(seed=77, sigma_w=sw, sigma_x0=sx, samples=S, with_feedforward=True, **common)
    _, loop = make_solver().closed_loop_batch(*pre, kp_tol=kp_tol, lim_tol=0.0, con_tol=con_tol, **loop_kw)
    for f in ("cost", "stats", "kp_err", "kp_stats", "lim_cost", "outcome", "con_max", "con_steps", "con_stats", "outcome_con"):
        assert np.array_equal(getattr(want, f), getattr(loop, f)), f
    assert np.array_equal(loop.X, old.X) and np.array_equal(loop.U, old.U)
    _, loop = make_solver().closed_loop_batch(*pre, con_tol=con_tol, **loop_kw)   # without tolerances: no outcome_con, no report
    for f in ("cost", "con_max", "con_steps", "con_stats"):
        assert np.array_equal(getattr(bare, f), getattr(loop, f)), f
    assert loop.outcome_con is None and loop.outcome is None and loop.kp_err is None
    _, loop = make_solver().closed_loop_batch(*pre, kp_tol=kp_tol, lim_tol=0.0, **loop_kw)   # without the new keyword: today's result
    for f in ("cost", "stats", "X", "U", "kp_err", "kp_stats", "lim_cost", "outcome"):
        assert np.array_equal(getattr(old, f), getattr(loop, f)), f
    assert loop.con_max is None and loop.con_steps is None and loop.con_stats is None and loop.outcome_con is None
    _, cv = make_solver().closed_loop_cov_batch(*pre, sigma_w=1e-3, sigma_x0=1e-2, want_Sigma=True, want_con=True, **common)
    for f in ("Sigma", "kp_Sigma", "kp_var", "u_var", "lim_z"):
        assert np.array_equal(getattr(cov_old, f), getattr(cv, f)), f
    assert np.array_equal(cv.con_var, cov.con_var) and np.array_equal(cv.con_z, cov.con_z)
    _, cv = make_solver().closed_loop_cov_batch(*pre, sigma_w=1e-3, sigma_x0=1e-2, **common)
    assert cv.con_var is None and cv.con_z is None and np.array_equal(cv.lim_z, cov_old.lim_z)
