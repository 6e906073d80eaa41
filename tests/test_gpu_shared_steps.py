"""Keypoints that share a timestep on the device.

Through the C ABI: the exact reductions of tests/shared_steps.py (a keypoint given twice, two precisions on one target, a zero keypoint) on
PosOrn 1st / 2nd order, PosOrnTime 1st / 2nd order and the hybrid joint + PosOrn sequence, recursive and AL, held to the parity proof against
the oracle's equivalent problem.  Shared steps always run on the generic kernels (plan_riccati: PlanIn::shared_steps), whatever the pins say:
every pin gives the bits of the generic pin, and a batch on each side of the plan's thresholds (3072 | 3073 instances for the forward pass,
4096 | 4097 for the lane grouping and the row sweep) gives every instance the bits it has in a batch of 13.

Through PyLQR: a SequentialSystem of a PosOrnPlannerSys and a JointSpacePlannerSys with both keypoints on the last step solves through
ILQRRecursive (its cost is the host evaluation of the sequence, which sums the sub-systems as the reference does) and AL_ILQR; BatchILQRCP
refuses it.  A plain System given two keypoints on one step keeps the last one given (System.cpp:78-80)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads
from tests import shared_steps as ss
from tests.helpers import GOLDEN, ROOT, golden

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "ilqr_planner_amd", "pylqr"))

URDF = os.path.join(GOLDEN, "panda_chain.urdf")
PINS = {
    "v1": dict(ILQR_HIP_PATH="v1"),
    "default": dict(ILQR_HIP_PATH="v2"),
    "mfma-dpp": dict(ILQR_HIP_PATH="v2", ILQR_SWEEP="mfma", ILQR_APPLY="dpp"),
    "rows-rows": dict(ILQR_HIP_PATH="v2", ILQR_SWEEP="rows", ILQR_APPLY="rows"),
    "wg": dict(ILQR_HIP_PATH="v2", ILQR_FWD="wg"),
    "dpp": dict(ILQR_HIP_PATH="v2", ILQR_FWD="dpp"),
}
SHAPES = ("C2", "C3", "C2nd", "C2ndal", "C4t1", "C4t1al", "C4", "C4al", "C2h")
B_SMALL = 13
BATCH_TEXT = "keypoints that share a timestep are not supported by the batch solvers"


def _pin(monkeypatch, pin):
    for k in ("ILQR_HIP_PATH", "ILQR_SWEEP", "ILQR_FWD", "ILQR_APPLY", "ILQR_CP", "ILQR_CP_SOLVE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PINS[pin].items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _same(a, b, tag):
    for k in ("X", "U", "K", "d", "cost", "iters", "ct", "at"):
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{tag}: {k} differs"


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("reduction", ss.REDUCTIONS)
def test_reduction_vs_oracle(ctx, monkeypatch, name, reduction):
    cfg, desc, inp, cfg_eq, inp_eq = ss.make_case(ctx, name, reduction, B_SMALL)
    _pin(monkeypatch, "default")
    ref, summ = ss.check_against_oracle(ctx, cfg, desc, inp, cfg_eq, inp_eq, f"{name} {reduction}")
    for pin in PINS:  # every pin runs the generic kernels on a shared step: the same bits
        _pin(monkeypatch, pin)
        p = ss.solve(ctx, cfg, desc, inp)
        try:
            _same(ss.results(p), ref, f"{name} {reduction} pin {pin}")
        finally:
            p.close()


def _tile(inp, n):
    reps = lambda a: np.ascontiguousarray(np.concatenate([a] * ((n + len(a) - 1) // len(a)))[:n])
    out = dict(inp, q0=reps(inp["q0"]), dq0=reps(inp["dq0"]), U0=reps(inp["U0"]), targets=[reps(t) for t in inp["targets"]])
    if "lambda0" in inp:
        out["lambda0"] = reps(inp["lambda0"])
    return out


@pytest.mark.parametrize("name", ("C3", "C4"))
@pytest.mark.parametrize("B", (3072, 3073, 4096, 4097))
def test_batch_thresholds(ctx, monkeypatch, name, B):
    """On each side of the plan's batch thresholds every instance has the bits it has in a batch of 13, under the pins that move there."""
    cfg, desc, inp, _, _ = ss.make_case(ctx, name, "sum", B_SMALL)
    _pin(monkeypatch, "default")
    p = ss.solve(ctx, cfg, desc, inp)
    small = ss.results(p)
    p.close()
    big_inp = _tile(inp, B)
    for pin in ("default", "wg", "dpp", "mfma-dpp", "rows-rows"):
        _pin(monkeypatch, pin)
        p = ss.solve(ctx, cfg, desc, big_inp)
        try:
            big = ss.results(p)
        finally:
            p.close()
        idx = np.arange(B) % B_SMALL
        for k in small:
            assert np.array_equal(big[k], small[k][idx], equal_nan=True), f"{name} B={B} pin {pin}: {k} differs from the batch of 13"


def test_batch_solvers_refuse(ctx):
    cfg, desc, inp, _, _ = ss.make_case(ctx, "C2", "double", 4)
    p = workloads.load_batch(ctx, desc, inp, 4)
    try:
        psi = workloads.psi_of(dict(kind="unitstep", K=2), cfg["T"], 7)
        with pytest.raises(RuntimeError, match=BATCH_TEXT):
            p.solve_batch_cp(psi, 2)
        with pytest.raises(RuntimeError, match=BATCH_TEXT):
            p.solve_batch(2)
        assert np.all(p.iters() == 0)
    finally:
        p.close()


# ---- PyLQR

def _hybrid_final(T=60, dt=0.05):
    from PyLQR.sim import KDLRobot
    from PyLQR.system import AngularKeypoint, JointSpacePlannerSys, PosOrnKeypoint, PosOrnPlannerSys, SequentialSystem

    g = golden()["cases"]["POS_ORN_SYS"]["problem"]
    dof = 7
    q0, dq0 = g["q0"], [0] * dof
    qMax = np.array([2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973])
    qMin = np.array([-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973])
    rbt = KDLRobot(URDF, "panda_link0", "panda_tip", q0, dq0)
    target_q = np.clip(np.asarray(q0) + np.random.default_rng(5).uniform(-0.3, 0.3, dof), qMin, qMax)
    sys1 = JointSpacePlannerSys(rbt, [AngularKeypoint(target_q, 0.1 * np.identity(dof), T - 1)], [1e-3] * dof, qMax, qMin, T, 1, dt)
    k2 = g["keypoints"][1]
    kp2 = PosOrnKeypoint(np.array(k2["pos"]), np.array(k2["orn"]), np.diag(k2["Qdiag"]), T - 1)
    sys2 = PosOrnPlannerSys(rbt, [kp2], [1e-4] * dof, qMax, qMin, T, 1, dt)
    return rbt, SequentialSystem(rbt, [sys1, sys2], [1e-6] * dof, T, 1), q0, target_q


def _host_cost(s, X, U):
    X, U = np.asarray(X), np.asarray(U)
    c = sum(float(np.asarray(s.cost(X[k], U[k], k)).reshape(-1)[0]) for k in range(len(U)))
    return c + float(np.asarray(s.cost_F(X[-1])).reshape(-1)[0])


def test_pylqr_sequence_on_final_step():
    from PyLQR.solver import AL_ILQR, BatchILQRCP, Constraint, ILQRRecursive
    from PyLQR.utils import PythonCallbackMessage, primitives

    T, dof = 60, 7
    rbt, s, q0, _ = _hybrid_final(T)
    cb = PythonCallbackMessage()
    u0 = np.zeros((T - 1, dof))
    X, F_X, U, K, k, cost = ILQRRecursive(s).solve(u0, 10, True, False, cb)
    X, U = np.asarray(X), np.asarray(U)
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(U))
    c = float(np.asarray(cost).reshape(-1)[-1])
    # the device's summed cost is the host evaluation of the sequence (SequentialSystem::cost sums its sub-systems' cost at each step)
    assert abs(c - _host_cost(s, X, U)) <= 1e-9 * max(1.0, abs(c)), (c, _host_cost(s, X, U))
    assert c < _host_cost(s, np.tile(np.asarray(q0), (T, 1)), u0)
    A, b = np.zeros((14, 14)), np.zeros(14)
    A[5, 5], b[5] = 1, 2.0
    cons, mult = [], []
    for _ in range(T - 1):
        cc = Constraint()
        cc.A, cc.b = A, b
        cons.append(cc)
        mult.append(b)
    Xa, _, Ua = AL_ILQR(s, cons, mult).solve(u0, 10, 5, .25, 1.1, True, False, cb)
    assert np.all(np.isfinite(np.asarray(Xa))) and np.all(np.isfinite(np.asarray(Ua)))
    assert _host_cost(s, Xa, Ua) < _host_cost(s, np.tile(np.asarray(q0), (T, 1)), u0)
    PSI = np.kron(primitives.build_psi_unitstep(T - 1, 2), np.identity(dof))
    with pytest.raises(RuntimeError, match=BATCH_TEXT):
        BatchILQRCP(s, PSI).solve(2, u0.reshape(-1), True, cb)


def test_pylqr_plain_system_keeps_last_keypoint():
    from PyLQR.sim import KDLRobot
    from PyLQR.solver import ILQRRecursive
    from PyLQR.system import PosOrnKeypoint, PosOrnPlannerSys
    from PyLQR.utils import PythonCallbackMessage

    g = golden()["cases"]["POS_ORN_SYS"]["problem"]
    T, dt, dof = 60, 0.05, 7
    q0, dq0 = g["q0"], [0] * dof
    qMax = np.array([np.pi] * dof) * 10
    k1, k2 = g["keypoints"][0], g["keypoints"][1]
    mk = lambda k, t: PosOrnKeypoint(np.array(k["pos"]), np.array(k["orn"]), np.diag(k["Qdiag"]), t)
    cb = PythonCallbackMessage()
    out = []
    for kps in ([mk(k1, T // 2), mk(k1, T - 1), mk(k2, T - 1)], [mk(k1, T // 2), mk(k2, T - 1)]):
        rbt = KDLRobot(URDF, "panda_link0", "panda_tip", q0, dq0)
        s = PosOrnPlannerSys(rbt, kps, [1e-5] * dof, qMax, -qMax, T, 1, dt)
        out.append([np.asarray(v) for v in ILQRRecursive(s).solve(np.zeros((T - 1, dof)), 8, True, False, cb)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_mixtures_device_against_host_loop(tmp_path):
    """tests/cpp/shared_steps_main.cpp on the product library: an object frame, a dead zone, a joint and two PosOrn keypoints with different
    targets on one step, solved through the lowering on the device and over the virtuals on the host (cost to 1e-5, U to 1e-6)."""
    lib_dir = os.path.join(ROOT, "ilqr_planner_amd")
    host = os.path.join(lib_dir, "csrc", "host")
    exe = str(tmp_path / "shared_steps")
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "shared_steps_main.cpp"), os.path.join(host, "ilqr_host.cpp"),
                           os.path.join(host, "ilqr_host_loop.cpp"), "-o", exe, "-L" + lib_dir, "-lilqr_hip", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, URDF], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"
