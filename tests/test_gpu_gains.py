"""Gains about a held plan on the device (ilqr_problem_gains): k_gains_prepare, k_kp_derivs and the sweep plan_riccati chooses -- k_backward_si_dpp
in its three forms, k_backward_mfma, k_backward_rows and the generic k_backward under their pins -- held to the checks of tests/gains.py: the
oracle's sweep about the plan each of the four solvers leaves (a), the bit property under every sweep pin (b), what must not move (c), the execution
tools on batch-solver plans (d), the state machine (e), the launches the profile counts, and the PyLQR layer.  Every system shape at T = 2, 3, 9,
25 on B = 13 and at B = 70 (more than one wave of 16-lane groups, ragged).  The host build of the generic kernels: tests/test_gains_cpu.py."""
import contextlib
import os

import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads
from tests import closed_loop_cov as cc
from tests import gains as gn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch

    torch.cuda.init()  # torch's device first, then the library's context (the device-pointer test hands torch tensors to the library)
    c = capi.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def pinned(pin):
    """pin: None (AUTO), "generic", or a sweep pin of ILQR_SWEEP (capi.BatchProblem applies the environment at every call)."""
    var, val = ("ILQR_HIP_PATH", "v1") if pin == "generic" else ("ILQR_SWEEP", pin)
    old = os.environ.get(var)
    if pin is not None:
        os.environ[var] = val
    try:
        yield
    finally:
        if pin is not None:
            if old is None:
                del os.environ[var]
            else:
                os.environ[var] = old


def sweep_pins(name):
    if name in ("shared", "C2hl"):   # the generic kernels only, whatever the pins say
        return (None, "generic")
    if name in gn.SI_SHAPES + ("chain3",):
        return (None, "siwave", "siwg", "siwgio", "generic")
    return (None, "mfma", "rows", "generic")


@pytest.mark.parametrize("name", gn.SHAPES + gn.EXTRA)
def test_oracle_sweep_about_riccati_plans(ctx, name):
    stats = gn.new_stats()
    for T in gn.HORIZONS:
        cfg, desc, inp, systems = gn.make_case(ctx, name, T)
        p = workloads.load_batch(ctx, desc, inp, gn.B)
        try:
            for source in ("zero", "rec") + (("al",) if name in gn.SHAPES else ()):
                gn.check_plan_gains(p, cfg, systems, source, f"{name} T={T} {source}", stats)
        finally:
            p.close()
    print(f"{name}: {stats['n']} instances, {stats['ill']} by the oracle's sensitivity (worst ratio {stats['worst_ratio']:.2f}); worst share of the "
          f"tolerance: K {stats['worst_K']:.3f}, d {stats['worst_d']:.3f}")


def test_oracle_sweep_and_bits_at_reg_1e_2(ctx):
    """gains.REG_CASE: the descriptor's reg away from its default, the oracle with the same reg (orc_set_constants)."""
    stats = gn.new_stats()
    gn.check_reg_case(ctx, stats)
    print(f"reg case: {stats}")
    assert stats["n"] >= gn.B


@pytest.mark.parametrize("name", gn.SHAPES)
def test_oracle_sweep_on_a_ragged_batch_of_70(ctx, name):
    stats = gn.new_stats()
    cfg, desc, inp, systems = gn.make_case(ctx, name, 9, gn.B_WIDE)
    p = workloads.load_batch(ctx, desc, inp, gn.B_WIDE)
    try:
        for source in ("zero", "rec"):
            gn.check_plan_gains(p, cfg, systems, source, f"{name} B={gn.B_WIDE} {source}", stats)
        gn.check_bits(p, inp, gn.bits_controls(inp), f"{name} B={gn.B_WIDE} bits")
    finally:
        p.close()
    print(f"{name}: {stats['n']} instances, {stats['ill']} by the oracle's sensitivity; worst share of the tolerance: K {stats['worst_K']:.3f}, "
          f"d {stats['worst_d']:.3f}")


@pytest.mark.parametrize("pin", [None, "generic"])
def test_instances_that_stopped_early_get_gains(ctx, pin):
    name, T, n = gn.STOP_CASE
    cfg, desc, inp, systems = gn.make_case(ctx, name, T)
    p = workloads.load_batch(ctx, desc, inp, gn.B)
    try:
        with pinned(pin):
            gn.check_plan_gains(p, dict(cfg, nit=n), systems, "stop", f"{name} T={T} stop {pin}", gn.new_stats(), want_stopped=True)
    finally:
        p.close()


# (shape, solver, K of the unit-step basis): Kw = 14 (narrow), Kw = 21 > 16 (the low-rank form) on constant-dt systems; BatchILQR on a constant-dt
# and on a time system
BATCH_PLANS = [("C2", "cp", 2), ("C2", "cp", 3), ("C2nd", "cp", 2), ("C2", "batch", 0), ("C4t1", "batch", 0)]


@pytest.mark.parametrize("name,solver,K", BATCH_PLANS)
def test_batch_solver_plans_get_gains_and_execute(ctx, name, solver, K):
    stats, cov = gn.new_stats(), cc.new_stats()
    for T in (9, 25):
        cfg, desc, inp, systems = gn.make_case(ctx, name, T)
        p = workloads.load_batch(ctx, desc, inp, gn.B)
        try:
            psi = workloads.psi_of(dict(kind="unitstep", K=K), T, p.dims.n_u) if solver == "cp" else None
            assert psi is None or (psi.shape[1] > 16) == (K == 3)
            tag = f"{name} T={T} {solver} K={K}"
            plan = gn.check_plan_gains(p, cfg, systems, solver, tag, stats, psi=psi)
            assert np.all(p.iters() >= 1), f"{tag}: the batch solver did not move the plan"
            if not cfg.get("ctimes"):   # (the time system's plan after three iterations is no plan to close a loop around)
                gn.check_execution(ctx, p, cfg, desc, systems, plan, tag, cov)
        finally:
            p.close()
    print(f"{name} {solver}: {stats['n']} instances, {stats['ill']} by the oracle's sensitivity; worst share of the tolerance: K {stats['worst_K']:.3f}, "
          f"d {stats['worst_d']:.3f}; covariance: {cov['ill']} of {cov['n']} outputs by their sensitivity")


@pytest.mark.parametrize("name", gn.SHAPES + gn.EXTRA)
def test_bit_property_under_every_sweep_pin(ctx, name):
    for T in gn.HORIZONS:
        cfg, desc, inp, _ = gn.make_case(ctx, name, T)
        p = workloads.load_batch(ctx, desc, inp, gn.B)
        try:
            U = gn.bits_controls(inp)
            K = {}
            for pin in sweep_pins(name):
                with pinned(pin):
                    gn.check_bits(p, inp, U, f"{name} T={T} pin {pin}")
                    p.set_controls(U)
                    p.solve_recursive(0, True, False)
                    p.gains()
                    K[pin] = p.K()
            for pin in ("siwave", "siwg", "siwgio"):   # the forms of k_backward_si_dpp: the same bytes as each other and as AUTO
                assert pin not in K or np.array_equal(K[pin], K[None]), f"{name} T={T}: the pin {pin} gives other bytes than AUTO"
        finally:
            p.close()


def test_the_halves_of_a_split_plan_get_the_same_gains(ctx):
    """B = 2048 on a time system: the matrix-core sweep as two halves on two streams (ilqr_plan.hpp: SPLIT_MIN_BATCH), joined to the context's stream."""
    Bn, T = 2048, 9
    cfg = dict(workloads.config("C4t1"), T=T, shape="C4t1")
    desc, inp = workloads.make_batch(ctx, cfg, B=Bn, seed=1)
    inp["U0"][:, :, -1] = np.sqrt(cfg["ctimes"][-1] / (T - 1))
    p = workloads.load_batch(ctx, desc, inp, Bn)
    try:
        p.solve_recursive(2, True, True)
        before = gn.snapshot(p, 2)
        p.gains()
        K, d = p.K(), p.d()
        gn.check_unmoved(before, gn.snapshot(p, 2), p.alpha(), "split")
        ctx.set_split(0)
        try:
            p.gains()
            assert np.array_equal(p.K(), K) and np.array_equal(p.d(), d), "the gains depend on the two-stream split"
        finally:
            ctx.set_split(1)
        idx = list(range(0, Bn, 128)) + [1023, 1024, Bn - 1]
        from tests.helpers import oracle_system_of_instance, panda_segs

        segs = panda_segs()
        systems = {i: oracle_system_of_instance(cfg, inp, i, segs) for i in idx}
        sub = [systems[i] for i in idx]
        gn.check_against_oracle(sub, before["U"][idx], K[idx], d[idx], before["status"][idx], "split", gn.new_stats())
    finally:
        p.close()


PROF = dict(rollout=0, backward=1, forward=2, other=3, apply=4)   # ILQR_PROF_*


@pytest.mark.parametrize("name,pin,source", [("C2", None, "rec"), ("C2", "generic", "rec"), ("C4", None, "rec"), ("C4", "rows", "zero"), ("C2", None, "batch"),
                                             ("C2", None, "cp")])
def test_a_gains_call_launches_one_sweep_and_no_rollout(ctx, name, pin, source):
    cfg, desc, inp, _ = gn.make_case(ctx, name, 9)
    p = workloads.load_batch(ctx, desc, inp, gn.B)
    ctx.profile(True)
    try:
        with pinned(pin):
            gn.make_plan(p, cfg, source, psi=workloads.psi_of(dict(kind="unitstep", K=2), 9, p.dims.n_u))
            ctx.synchronize()
            ctx.profile_reset()
            p.gains()
            ctx.synchronize()
        n = {k: ctx.profile_get(v)[1] for k, v in PROF.items()}
        assert n["rollout"] == 0 and n["forward"] == 0 and n["apply"] == 0, f"a gains() call launched {n}"
        assert n["backward"] == 1, f"a gains() call launched {n}"   # (with the profile on no plan splits)
        assert n["other"] >= 1
    finally:
        ctx.profile(False)
        ctx.profile_reset()
        p.close()


def test_state_machine_and_error_texts(ctx):
    gn.check_state_machine(ctx, batch_solvers=True, psi_of=workloads.psi_of)
    with pinned("generic"):
        gn.check_state_machine(ctx, batch_solvers=True, psi_of=workloads.psi_of)


def test_device_pointer_entry_points_accept_the_plan(ctx):
    import torch

    cfg, desc, inp, _ = gn.make_case(ctx, "C2", 9)
    p = workloads.load_batch(ctx, desc, inp, gn.B)
    try:
        p.solve_batch(2, True)
        p.gains()
        host = p.closed_loop(samples=2)
        dev = torch.device("cuda:0")
        cost = torch.zeros((p.B, 2), dtype=torch.float64, device=dev)
        X = torch.zeros((p.B, 2, p.T, p.dims.n_x), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        p.closed_loop_dev(2, None, None, False, cost.data_ptr(), X.data_ptr(), None)
        ctx.synchronize()
        assert np.array_equal(cost.cpu().numpy(), host[0]) and np.array_equal(X.cpu().numpy(), host[1])
    finally:
        p.close()


def _pylqr_case(ctx, T=9):
    """The C2 case as a PyLQR System, with the unit-step basis of the C5 configuration."""
    import sys

    from tests.helpers import GOLDEN, ROOT

    sys.path.insert(0, os.path.join(ROOT, "ilqr_planner_amd", "pylqr"))
    from PyLQR.sim import KDLRobot
    from PyLQR.system import PosOrnKeypoint, PosOrnPlannerSys

    cfg, desc, inp, systems = gn.make_case(ctx, "C2", T)
    qMax = np.full(7, 10 * np.pi)
    rbt = KDLRobot(os.path.join(GOLDEN, "panda_chain.urdf"), "panda_link0", "panda_tip", list(inp["q0"][0]), [0.0] * 7)
    kps = [PosOrnKeypoint(np.array(tg[0][0:3]), np.array(tg[0][3:7]), np.diag(cfg["Qdiag"][k]), int(inp["kp_t"][k])) for k, tg in enumerate(inp["targets"])]
    sys_ = PosOrnPlannerSys(rbt, kps, list(workloads.control_weights(cfg, 7)), qMax, -qMax, T, 1, cfg["dt"])
    psi = workloads.psi_of(dict(kind="unitstep", K=2), T, 7)
    return cfg, desc, inp, sys_, psi


def test_pylqr_batch_cp_plan_gains_and_closed_loops_equal_the_c_abi(ctx):
    cfg, desc, inp, sys_, psi = _pylqr_case(ctx)
    from PyLQR.solver import BatchILQR, BatchILQRCP

    n = gn.iterations(cfg)
    u0 = inp["U0"].reshape(gn.B, -1)
    common = dict(q0=inp["q0"], kp_targets=list(inp["targets"]))
    sw, sx = cc.sigmas(7)
    for solver, solve in ((BatchILQRCP(sys_, psi), lambda p: p.solve_batch_cp(psi, n, True)), (BatchILQR(sys_), lambda p: p.solve_batch(n, True))):
        p = workloads.load_batch(ctx, desc, inp, gn.B)
        try:
            solve(p)
            alpha = p.alpha()
            p.gains()
            plan = dict(X=p.X(), U=p.U(), K=p.K(), d=p.d(), cost=p.cost())
            x0, w = gn.cl.perturbations(plan, 3, seed=11)
            loop = p.closed_loop(x0, w, with_feedforward=True)
            cov = cc.call(p, sw, sx)
        finally:
            p.close()
        assert solver.solve_batch(n, u0, True, **common).K.size == 0          # without the keyword: no gains, as before
        res = solver.solve_batch(n, u0, True, plan_gains=True, **common)
        assert np.array_equal(res.K, plan["K"]) and np.array_equal(res.d, plan["d"]), "solve_batch(plan_gains=True) differs from ilqr_problem_gains"
        assert np.array_equal(res.X, plan["X"]) and np.array_equal(res.U, plan["U"]) and np.array_equal(res.alpha, alpha)
        res, got = solver.closed_loop_batch(n, u0, True, x0=x0, w=w, with_feedforward=True, **common)
        assert np.array_equal(res.K, plan["K"])
        assert np.array_equal(got.cost, loop[0]) and np.array_equal(got.X, loop[1]) and np.array_equal(got.U, loop[2])
        _, gcov = solver.closed_loop_cov_batch(n, u0, True, sigma_w=sw, sigma_x0=sx, want_Sigma=True, **common)
        for f in cc.FIELDS:
            assert np.array_equal(getattr(cov, f), getattr(gcov, f)), f


def test_pylqr_riccati_solvers_keep_their_results_without_the_keyword(ctx):
    cfg, desc, inp, sys_, _ = _pylqr_case(ctx)
    from PyLQR.solver import ILQRRecursive

    n = gn.iterations(cfg)
    common = dict(q0=inp["q0"], kp_targets=list(inp["targets"]))
    p = workloads.load_batch(ctx, desc, inp, gn.B)
    try:   # the C-ABI solve: what the parent's solve_batch returns (tests/test_gpu_closed_loop.py holds the two equal)
        p.solve_recursive(n, True, True)
        want = dict(X=p.X(), U=p.U(), K=p.K(), d=p.d(), cost=p.cost(), alpha=p.alpha())
        p.gains()
        Kg, dg = p.K(), p.d()
    finally:
        p.close()
    solver = ILQRRecursive(sys_)
    stored = solver.solve_batch(inp["U0"], n, True, True, **common)   # the call as it was written before the keyword existed
    for f, v in want.items():
        assert np.array_equal(getattr(stored, f), v), f"solve_batch without plan_gains: {f} changed"
    off = solver.solve_batch(inp["U0"], n, True, True, plan_gains=False, **common)
    for f in want:
        assert getattr(off, f).tobytes() == getattr(stored, f).tobytes(), f
    on = solver.solve_batch(inp["U0"], n, True, True, plan_gains=True, **common)
    assert np.array_equal(on.K, Kg) and np.array_equal(on.d, dg)
    assert np.array_equal(on.X, want["X"]) and np.array_equal(on.alpha, want["alpha"])
    assert not np.array_equal(on.K, want["K"]), "the plan's gains equal the solver's: the solve moved nothing in its last iteration"
    x0, w = gn.cl.perturbations(want, 2, seed=3)
    _, a = solver.closed_loop_batch(inp["U0"], n, True, True, x0=x0, w=w, **common)
    _, b = solver.closed_loop_batch(inp["U0"], n, True, True, x0=x0, w=w, plan_gains=False, **common)
    _, c = solver.closed_loop_batch(inp["U0"], n, True, True, x0=x0, w=w, plan_gains=True, **common)
    assert a.cost.tobytes() == b.cost.tobytes() and a.X.tobytes() == b.X.tobytes()
    assert not np.array_equal(a.U, c.U), "plan_gains = True leaves the closed loop on the solver's gains"
