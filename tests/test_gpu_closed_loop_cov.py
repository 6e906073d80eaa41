"""Analytic covariance of the closed loop on the device (ilqr_problem_closed_loop_cov): the row kernel k_cl_cov_rows where plan_closed_loop_cov
chooses it and the generic k_cl_cov under the pin (and for the 3-joint chain), with k_cl_cov_kp behind both -- held to the checks of
tests/closed_loop_cov.py: the NumPy recursion (1), the Jacobian against the oracle's step (2), the exact properties (3), the sampled path (4),
refusals and interfaces (5).  Every system shape of tests/closed_loop.py at T = 2, 3, 9, 25 on B = 13, ragged against the 4 instances of a
wave.  The host build of the generic kernel: tests/test_closed_loop_cov_cpu.py."""
import os
import sys

import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads
from tests import closed_loop as cl
from tests import closed_loop_cov as cc
from tests.helpers import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch

    torch.cuda.init()  # torch's device first, then the library's context (the device-pointer test hands torch tensors to the library)
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", cl.SHAPES + cl.EXTRA)
def test_recursion_jacobian_and_exact_properties_on_both_kernels(ctx, name):
    stats = cc.new_stats()
    for T in cc.HORIZONS:
        print(cc.check_case(ctx, name, T, stats=stats, pins=(False, True)), flush=True)
    print(f"{name}: {stats['ill']} of {stats['n']} outputs by their sensitivity (worst ratio {stats['worst_ratio']:.2f}); worst deviations within the "
          "bound: " + ", ".join(f"{f} {stats[f]:.3e}" for f in cc.FIELDS) + f"; pinned = planned bit for bit on {stats.get('same', 0)} plans, "
          f"not on {stats.get('differ', 0)}")
    # Which kernel ran is seen in the last bits: the two sum in different orders.  A narrow chain takes the generic kernel with or without the
    # pin; every 7-joint shape must reach the row kernel without it.  C1j cannot show it: its gains are exactly diagonal (joint-space
    # keypoints with diagonal precisions), so Sigma stays diagonal, every sum has one non-zero term and both orders give the same bits.
    if name == "chain3":
        assert stats.get("differ", 0) == 0
    elif name != "C1j":
        assert stats.get("differ", 0) > 0, f"{name}: the unpinned calls return the generic kernel's bits at every horizon: k_cl_cov_rows was not reached"


@pytest.mark.parametrize("name", ["C2", "C2nd", "C4", "chain3"])
def test_cut_out_reproduces_the_large_call(ctx, name):
    cc.check_cut_out(ctx, name)
    with cl.generic_pin():
        cc.check_cut_out(ctx, name)


@pytest.mark.parametrize("name", cc.SAMPLED)
def test_sample_covariance_converges_to_sigma(ctx, name):
    for pin in (False, True):
        with (cl.generic_pin() if pin else cc._nothing()):
            worst, worst_open = cc.check_sampled(ctx, name)
        print(f"{name}{' generic' if pin else ''}: within {worst:.2f} standard deviations (open loop: {worst_open:.1f})")


def _torch_call(p, sw, sx, wants):
    import torch

    dev = torch.device("cuda:0")
    nx, nk = p.dims.n_x, p.n_kp
    shapes = dict(Sigma=(p.B, p.T, nx, nx), kp_Sigma=(p.B, nk, nx, nx), kp_var=(p.B, nk, 5), u_var=(p.B, p.T - 1, p.dims.n_u), lim_z=(p.B,))
    out = {f: (torch.zeros(shapes[f], dtype=torch.float64, device=dev) if wants[f] else None) for f in cc.FIELDS}
    torch.cuda.synchronize()
    p.closed_loop_cov_dev(sw, sx, **{f + "_ptr": (out[f].data_ptr() if out[f] is not None else None) for f in cc.FIELDS})
    p.ctx.synchronize()
    return capi.ClosedLoopCov(**{f: (t.cpu().numpy() if t is not None else None) for f, t in out.items()})


def test_error_texts_and_device_pointers(ctx):
    cc.check_interfaces(ctx, _torch_call, batch_solver=True, size_refusals=True)
    with cl.generic_pin():
        cc.check_interfaces(ctx, _torch_call)


def test_pylqr_closed_loop_cov_batch_equals_the_c_abi(ctx):
    sys.path.insert(0, os.path.join(ROOT, "ilqr_planner_amd", "pylqr"))
    from PyLQR.sim import KDLRobot
    from PyLQR.solver import AL_ILQR, Constraint, ILQRRecursive
    from PyLQR.system import PosOrnKeypoint, PosOrnPlannerSys

    T = 9
    for name in ("C2", "C3"):
        cfg, desc, inp, _ = cl.make_case(ctx, name, T)
        p = cl.solve(ctx, cfg, desc, inp)
        try:
            sw, sx = cc.sigmas(7)
            want = cc.call(p, sw, sx)
            scalar = cc.call(p, 1e-3, None)
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
        common = dict(q0=q0, kp_targets=list(inp["targets"]))
        _, cov = solver.closed_loop_cov_batch(*pre, sigma_w=sw, sigma_x0=sx, want_Sigma=True, **common)
        for f in cc.FIELDS:
            assert np.array_equal(getattr(want, f), getattr(cov, f)), f"{name}: {f}"
        _, cov = solver.closed_loop_cov_batch(*pre, sigma_w=1e-3, **common)
        assert cov.Sigma is None
        for f in cc.FIELDS[1:]:
            assert np.array_equal(getattr(scalar, f), getattr(cov, f)), f"{name}: {f} with a scalar sigma"
        with pytest.raises(RuntimeError, match="sigma_w and sigma_x0 must be a scalar or have nb_state_var entries"):
            solver.closed_loop_cov_batch(*pre, sigma_w=[1e-3, 1e-3], **common)
