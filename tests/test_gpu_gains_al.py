"""Gains with the AL constraint terms about a held plan on the device (ilqr_problem_gains_al): k_gains_prepare, k_gains_al_weights where the sweep
reads stored weights, k_kp_derivs and the AL sweep plan_riccati chooses -- k_backward_si_dpp in its forms (it forms its weights itself),
k_backward_mfma, k_backward_rows and the generic k_backward under their pins -- held to the checks of tests/gains_al.py: the oracle's AL sweep
about the plans a 0-iteration solve, an AL solve and Batch-CP leave (a), the bit property under every sweep pin (b), what must not move (c), the
degenerate rows (d), the execution tools (e), the state machine, refusals and launch counts (f), the PyLQR layer and the penalty helper (g).
B = 13 at T = 2, 3, 9, 25; B = 70 (more than one wave of 16-lane groups, ragged); one split case at B = 2048.  The host build of the generic
kernels: tests/test_gains_al_cpu.py."""
import contextlib
import os
import sys

import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads
from tests import closed_loop as cl
from tests import closed_loop_cov as cc
from tests import gains as gn
from tests import gains_al as ga
from tests.helpers import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

PROF = dict(rollout=0, backward=1, forward=2, other=3, apply=4)   # ILQR_PROF_*

# every pin on every case: a pin that does not apply to a shape acts as AUTO (ilqr_plan.hpp), the forms of k_backward_si_dpp give AUTO's bytes
PINS = (None, "siwave", "siwg", "siwgio", "siwgprep", "mfma", "rows", "generic")
SI_FORMS = ("siwave", "siwg", "siwgio", "siwgprep")
CP_CASES = ("C3-m1", "C3-m4", "C3-m5-dense", "C2ndal-m2-control")   # constant-dt systems: the unit-step basis of the C5 configuration
WIDE_CASES = tuple(c for c in ga.CASES if c != "chain3-m1")


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


def _line(stats):
    return (f"{stats['n']} instances, {stats['ill']} by the oracle's sensitivity (worst ratio {stats['worst_ratio']:.2f}), {stats['skipped']} skipped; "
            f"worst share of the tolerance: K {stats['worst_K']:.3f}, d {stats['worst_d']:.3f}")


@pytest.mark.parametrize("T", ga.HORIZONS)
@pytest.mark.parametrize("case", ga.CASES)
def test_oracle_al_sweep_about_riccati_plans(ctx, case, T):
    stats = ga.new_stats()
    cfg, desc, inp, systems = ga.make_case(ctx, case, T)
    p = workloads.load_batch(ctx, desc, inp, ga.B)
    try:
        for source in ("zero", "al"):
            ga.restore(p, inp)
            ga.check_plan_gains(p, cfg, inp, systems, source, ga.penalties(cfg), f"{case} T={T} {source}", stats)
    finally:
        p.close()
    print(f"{case} T={T}: {_line(stats)}")


def test_oracle_al_sweep_and_bits_at_reg_1e_2(ctx):
    """gains_al.REG_CASE: the descriptor's reg away from its default, the oracle with the same reg (orc_set_constants)."""
    stats = ga.new_stats()
    ga.check_reg_case(ctx, stats)
    print(f"reg case: {_line(stats)}")
    assert stats["n"] >= 2 * ga.B


@pytest.mark.parametrize("T", (9, 25))
@pytest.mark.parametrize("case", CP_CASES)
def test_oracle_al_sweep_about_batch_cp_plans(ctx, case, T):
    stats = ga.new_stats()
    cfg, desc, inp, systems = ga.make_case(ctx, case, T)
    p = workloads.load_batch(ctx, desc, inp, ga.B)
    try:
        psi = workloads.psi_of(dict(kind="unitstep", K=2), T, p.dims.n_u)
        plan = ga.check_plan_gains(p, cfg, inp, systems, "cp", ga.penalties(cfg), f"{case} T={T} cp", stats, psi=psi)
        assert np.all(p.iters() >= 1) and np.any(plan["lam"] > 0), f"{case} T={T}: the Batch-CP plan or its multipliers test nothing"
    finally:
        p.close()
    print(f"{case} T={T} cp: {_line(stats)}")


@pytest.mark.parametrize("case", WIDE_CASES)
def test_oracle_al_sweep_and_bits_on_a_ragged_batch_of_70(ctx, case):
    stats = ga.new_stats()
    cfg, desc, inp, systems = ga.make_case(ctx, case, 9, ga.B_WIDE)
    pens = ga.penalties(cfg)
    p = workloads.load_batch(ctx, desc, inp, ga.B_WIDE)
    try:
        ga.check_plan_gains(p, cfg, inp, systems, "al", pens[1:], f"{case} B={ga.B_WIDE} al", stats)
        lam, U = ga.multipliers_and_controls(p, cfg, inp)
        for pin in (None, "generic"):
            with pinned(pin):
                ga.check_bits(p, inp, lam, U, pens[1], f"{case} B={ga.B_WIDE} pin {pin}")
    finally:
        p.close()
    print(f"{case} B={ga.B_WIDE}: {_line(stats)}")


@pytest.mark.parametrize("T", ga.HORIZONS)
@pytest.mark.parametrize("case", ga.CASES)
def test_bit_property_under_every_sweep_pin_and_degenerate_rows(ctx, case, T):
    cfg, desc, inp, _ = ga.make_case(ctx, case, T)
    pens = ga.penalties(cfg)
    p = workloads.load_batch(ctx, desc, inp, ga.B)
    try:
        lam, U = ga.multipliers_and_controls(p, cfg, inp)
        K = {}
        for pin in PINS:
            with pinned(pin):
                for pen in pens:
                    K[pin, pen] = ga.check_bits(p, inp, lam, U, pen, f"{case} T={T} pin {pin} pen={pen:.6g}")[0]
                ga.check_degenerate(p, cfg, inp, U, f"{case} T={T} pin {pin}")
        fin = (p.status() & 1) == 0
        for pin in SI_FORMS:   # the forms of k_backward_si_dpp: the same bytes as each other and as AUTO
            for pen in pens:
                assert np.array_equal(K[pin, pen][fin], K[None, pen][fin]), f"{case} T={T}: the pin {pin} gives other bytes than AUTO"
        if T >= 9:
            ga.check_rows_matter(p, cfg, inp, lam, U, pens[1], f"{case} T={T}")
            with pinned("generic"):
                ga.check_rows_matter(p, cfg, inp, lam, U, pens[1], f"{case} T={T} generic")
            ga.check_penalty_of_last_update(p, cfg, inp, f"{case} T={T}")
    finally:
        p.close()


@pytest.mark.parametrize("pin", [None, "generic"])
@pytest.mark.parametrize("case", ga.CASES)
def test_execution_on_the_al_gains(ctx, case, pin):
    rep, cov, worst = cl.new_stats(), cc.new_stats(), dict(con_max=0.0, con_var=0.0)
    for T in (9, 25):
        cfg, desc, inp, systems = ga.make_case(ctx, case, T)
        p = workloads.load_batch(ctx, desc, inp, ga.B)
        try:
            with pinned(pin):
                plan = ga.check_plan_gains(p, cfg, inp, None, "al", ga.penalties(cfg)[1:], f"{case} T={T} al {pin}", ga.new_stats())
                ga.check_execution(ctx, p, cfg, desc, inp, systems, plan, case, f"{case} T={T} al {pin}", rep, cov, worst)
        finally:
            p.close()
    print(f"{case} {pin}: replay {rep['n']} samples, {rep['ill']} by their sensitivity; covariance {cov['ill']} of {cov['n']} outputs by their sensitivity; "
          f"con_max at most {worst['con_max']:.3e} of its bound, con_var at most {worst['con_var']:.3e} relative")


def test_the_halves_of_a_split_plan_get_the_same_al_gains(ctx):
    """B = 2048 on PosOrnTime-2 with 16 rows: the matrix-core AL sweep as two halves on two streams (ilqr_plan.hpp: SPLIT_MIN_BATCH), Is and lambda
    of each half at its own offset, joined to the context's stream."""
    case, T, Bn = ga.SPLIT
    cfg, desc, inp, _ = ga.make_case(ctx, case, T, Bn)
    al = cfg["al"]
    pen = ga.penalties(cfg)[1]
    p = workloads.load_batch(ctx, desc, inp, Bn)
    try:
        p.solve_al(2, al["lag"], al["penalty"], al["scaling"], True, True)
        before = gn.snapshot(p, 2)
        p.gains_al(pen)
        K, d = p.K(), p.d()
        gn.check_unmoved(before, gn.snapshot(p, 2), p.alpha(), "split")
        ctx.set_split(0)
        try:
            p.gains_al(pen)
            assert np.array_equal(p.K(), K, equal_nan=True) and np.array_equal(p.d(), d, equal_nan=True), "the AL gains depend on the two-stream split"
        finally:
            ctx.set_split(1)
        idx = list(range(0, Bn, 128)) + [1023, 1024, Bn - 1]
        from tests.helpers import oracle_system_of_instance, panda_segs

        segs = panda_segs()
        sub = [oracle_system_of_instance(cfg, inp, i, segs) for i in idx]
        cut = dict(A=inp["A"], b=inp["b"])
        ga.check_against_oracle(sub, cut, before["U"][idx], before["lam"][idx], pen, K[idx], d[idx], before["status"][idx], "split", ga.new_stats())
    finally:
        p.close()


# (case, pin, launches charged to OTHER): k_gains_prepare and k_kp_derivs, and k_gains_al_weights where the sweep reads stored weights -- not for the
# fused k_backward_si_dpp (C3 with up to 4 shared state rows under AUTO), which forms them itself
LAUNCHES = [("C3-m1", None, 2), ("C3-m4", None, 2), ("C3-m1", "generic", 3), ("C3-m5-dense", None, 3), ("C2ndal-m2-control", "rows", 3), ("C4al-m16", None, 3)]


@pytest.mark.parametrize("case,pin,n_other", LAUNCHES)
def test_a_gains_al_call_launches_one_sweep_and_no_rollout(ctx, case, pin, n_other):
    cfg, desc, inp, _ = ga.make_case(ctx, case, 9)
    p = workloads.load_batch(ctx, desc, inp, ga.B)
    ctx.profile(True)
    try:
        with pinned(pin):
            ga.make_plan(p, cfg, inp, "al")
            ctx.synchronize()
            ctx.profile_reset()
            p.gains_al(ga.penalties(cfg)[1])
            ctx.synchronize()
        n = {k: ctx.profile_get(v)[1] for k, v in PROF.items()}
        assert n["rollout"] == 0 and n["forward"] == 0 and n["apply"] == 0, f"a gains_al() call launched {n}"
        assert n["backward"] == 1 and n["other"] == n_other, f"a gains_al() call launched {n}"
    finally:
        ctx.profile(False)
        ctx.profile_reset()
        p.close()


def test_state_machine_and_error_texts(ctx):
    ga.check_state_machine(ctx, batch_solvers=True, psi_of=workloads.psi_of)
    with pinned("generic"):
        ga.check_state_machine(ctx, batch_solvers=True, psi_of=workloads.psi_of)


def test_device_pointer_entry_points_accept_the_al_gains(ctx):
    import torch

    cfg, desc, inp, _ = ga.make_case(ctx, "C3-m4", 9)
    p = workloads.load_batch(ctx, desc, inp, ga.B)
    try:
        ga.make_plan(p, cfg, inp, "zero")
        p.gains_al(cfg["al"]["penalty"])
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


@pytest.mark.parametrize("nit", [ga.NIT, ga.NIT + 1])   # a multiple of the lag and not
def test_pylqr_al_gains_penalty_equals_the_c_abi(ctx, nit):
    sys.path.insert(0, os.path.join(ROOT, "ilqr_planner_amd", "pylqr"))
    from PyLQR.sim import KDLRobot
    from PyLQR.solver import AL_ILQR, BatchILQR, Constraint, ILQRRecursive
    from PyLQR.system import PosOrnKeypoint, PosOrnPlannerSys

    ga.check_final_penalty(AL_ILQR.final_penalty)
    T, S, case = 9, 3, "C3-m4"
    cfg, desc, inp, _ = ga.make_case(ctx, case, T)
    al = cfg["al"]
    pen = AL_ILQR.final_penalty(nit, al["lag"], al["penalty"], al["scaling"])
    assert pen == ga.final_penalty(nit, al["lag"], al["penalty"], al["scaling"])
    sw, sx = ga.con.sigmas_of(case, 7, T)
    p = workloads.load_batch(ctx, desc, inp, ga.B)
    try:
        p.solve_al(nit, al["lag"], al["penalty"], al["scaling"], True, True)
        solved = dict(X=p.X(), U=p.U(), K=p.K(), d=p.d(), cost=p.cost(), alpha=p.alpha())
        old_loop = p.closed_loop_noise(S, 77, sw, sx, with_feedforward=False, want_X=True, want_U=True)
        p.gains_al(pen)
        Kg, dg = p.K(), p.d()
        loop = p.closed_loop_noise(S, 77, sw, sx, with_feedforward=False, want_X=True, want_U=True)
        cov = p.closed_loop_cov_con(1e-3, 1e-2)
        lam, U = p.lam(), solved["U"]
        for q in (pen, al["penalty"]):   # (b) at the final penalty of this iteration count
            ga.check_bits(p, inp, lam, U, q, f"{case} nit={nit} pen={q:.6g}")
    finally:
        p.close()
    assert not np.array_equal(Kg, solved["K"])
    qMax = np.full(7, 10 * np.pi)
    rbt = KDLRobot(os.path.join(GOLDEN, "panda_chain.urdf"), "panda_link0", "panda_tip", list(inp["q0"][0]), [0.0] * 7)
    kps = [PosOrnKeypoint(np.array(tg[0][0:3]), np.array(tg[0][3:7]), np.diag(cfg["Qdiag"][k]), int(inp["kp_t"][k])) for k, tg in enumerate(inp["targets"])]
    sys_ = PosOrnPlannerSys(rbt, kps, list(workloads.control_weights(cfg, 7)), qMax, -qMax, T, 1, cfg["dt"])
    cons = []
    for _ in range(T - 1):
        c = Constraint()
        c.A, c.b = inp["A"], inp["b"]
        cons.append(c)
    # a solver per call: AL_ILQR keeps the multipliers of its last solve, as the reference's member does
    make_solver = lambda: AL_ILQR(sys_, cons, [inp["lambda0"][0, k] for k in range(T - 1)])  # noqa: E731
    pre = (inp["U0"], nit, al["lag"], al["penalty"], al["scaling"], True, True)
    common = dict(q0=inp["q0"], kp_targets=list(inp["targets"]))
    stored = make_solver().solve_batch(*pre, **common)             # the call as it was written before the keyword existed
    kept = ("X", "U", "cost", "alpha")   # (AL_ILQR.solve_batch returns no gains of its own: the reference's solve returns X, fX, U)
    for f in kept:
        assert np.array_equal(getattr(stored, f), solved[f]), f"solve_batch without al_gains_penalty: {f} changed"
    assert stored.K.size == 0 and stored.d.size == 0
    off = make_solver().solve_batch(*pre, al_gains_penalty=None, **common)
    for f in kept + ("K", "d"):
        assert getattr(off, f).tobytes() == getattr(stored, f).tobytes(), f
    on = make_solver().solve_batch(*pre, al_gains_penalty=pen, **common)
    assert np.array_equal(on.K, Kg) and np.array_equal(on.d, dg), "solve_batch(al_gains_penalty=pen) differs from ilqr_problem_gains_al"
    assert np.array_equal(on.X, solved["X"]) and np.array_equal(on.U, solved["U"]) and np.array_equal(on.alpha, solved["alpha"])
    loop_kw = dict(seed=77, sigma_w=sw, sigma_x0=sx, samples=S, with_feedforward=False, **common)
    _, a = make_solver().closed_loop_batch(*pre, **loop_kw)
    assert np.array_equal(a.cost, old_loop.cost) and np.array_equal(a.X, old_loop.X)
    res, b = make_solver().closed_loop_batch(*pre, al_gains_penalty=pen, **loop_kw)
    assert np.array_equal(res.K, Kg)
    assert np.array_equal(b.cost, loop.cost) and np.array_equal(b.X, loop.X) and np.array_equal(b.U, loop.U)
    assert not np.array_equal(a.U, b.U), "al_gains_penalty leaves the closed loop on the solver's gains"
    _, cv = make_solver().closed_loop_cov_batch(*pre, sigma_w=1e-3, sigma_x0=1e-2, want_con=True, al_gains_penalty=pen, **common)
    assert np.array_equal(cv.con_var, cov.con_var) and np.array_equal(cv.con_z, cov.con_z)
    for bad in (-1.0, float("nan")):
        with pytest.raises(RuntimeError, match="al_gains_penalty must be finite and >= 0"):
            make_solver().solve_batch(*pre, al_gains_penalty=bad, **common)
    # the field is AL_ILQR's: the other classes have no keyword
    for other, args in ((ILQRRecursive(sys_), (inp["U0"], nit, True, True)), (BatchILQR(sys_), (nit, inp["U0"].reshape(ga.B, -1), True))):
        with pytest.raises(TypeError):
            other.solve_batch(*args, al_gains_penalty=pen, **common)

