"""The device on chains that are not the Panda (tests/golden/chains/gen7.urdf, gen4.urdf: joint axes along x, y, -z and oblique ones, origins
with roll, pitch and yaw, fixed joints before, between and behind the moving ones).  Kinematics are held to the high-precision reference of
tests/kinematics_reference.py, not to the oracle (tests/test_kinematics_cpu.py holds the oracle to the same reference); the solvers are held
to the oracle through the unchanged parity gate of tests/parity_proof.py.  Small on purpose: B <= 32, T = 30 (40 for the batch solvers), 5 or 6
iterations."""
import os
import sys

import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads
from tests import kinematics_reference as kr
from tests import narrow_chain as nc
from tests import parity_proof as pp
from tests.helpers import (GENERAL_CHAINS, GOLDEN, ROOT, TOOL_FRAMES, general_chain, general_chain_text, object_frames, oracle_solve_instance,
                           oracle_system_of_instance, orc)

pytestmark = pytest.mark.gpu

T, B, NIT = 30, 24, 6
GENERAL_SWEEP = {"C2nd", "C4t1", "C4", "C2ndal"}  # the workloads below on the 2nd-order / time systems' sweeps
# the kernel sets of tests/test_gpu_parity.py's hip_path: v2 (default), v1 (generic lane-per-instance kernels), v2rows (the second sweep of the
# 2nd-order / time systems forced at test sizes), v2wg (the second forward pass of the single-integrator systems forced at test sizes)
PATHS = {"v2": dict(ILQR_HIP_PATH="v2"), "v1": dict(ILQR_HIP_PATH="v1"), "v2rows": dict(ILQR_HIP_PATH="v2", ILQR_SWEEP="rows", ILQR_APPLY="rows"),
         "v2wg": dict(ILQR_HIP_PATH="v2", ILQR_FWD="wg")}


def _paths(name):
    return ["v2", "v1", "v2rows" if name in GENERAL_SWEEP else "v2wg"]


@pytest.fixture
def hip_path(request, monkeypatch):
    """One of PATHS (indirect parameter; "v2" where a test does not name one).  Test plumbing of capi.py: the variables become
    ilqr_ctx_set_crosscheck before every solve; the library reads no environment."""
    for k in ("ILQR_HIP_PATH", "ILQR_CP_SOLVE", "ILQR_CP", "ILQR_SWEEP", "ILQR_FWD", "ILQR_APPLY"):
        monkeypatch.delenv(k, raising=False)
    path = getattr(request, "param", "v2")
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    return path


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _tool(tool):
    rpy, xyz = TOOL_FRAMES[tool]
    return rpy or (0, 0, 0), xyz or (0, 0, 0)


def _ref_chain(name):
    return kr.read_chain(general_chain_text(name), *GENERAL_CHAINS[name][1:])


# ---- kinematics against the reference


@pytest.mark.parametrize("name,tool", [(n, t) for n in ("gen7", "gen4") for t in ("identity", "rotated")])
def test_fk_batch_vs_reference(ctx, name, tool):
    """ilqr_fk_batch on 128 configurations, uniform in +-3.1: position, signed quaternion and Jacobian within 1e-12 absolute of the
    reference.  A sample whose branch decision lies within 1e-9 of its boundary is compared up to sign; at most 2 % may be.  On the
    reference's side (seed 9, known without a device): no sample that close, and branches (trace, R00, R11, R22) 42 / 21 / 28 / 37 on gen4
    with the rotated tool.  Measured on an MI355X: 8.9e-16 at worst."""
    n = 128
    ch, _ = general_chain(name, tool)
    dof = ch["dof"]
    desc = capi.make_desc(kind=capi.SYS_POS_ORN, nb_deriv=1, horizon=2, dt=0.1, R_diag=[1e-5] * dof, chain=ch, kp_timesteps=[], kp_Q=[])
    q = np.random.default_rng(9).uniform(-3.1, 3.1, (n, dof))
    pos, quat, jac = ctx.fk_batch(desc, q)
    ref = _ref_chain(name)
    branches, near, worst = [0] * 4, 0, 0.0
    for i in range(n):
        r = kr.fk(ref, q[i], *_tool(tool))
        branches[r["branch"]] += 1
        near += r["margin"] <= kr.BOUNDARY
        worst = max(worst, np.abs(pos[i] - r["pos"]).max(), np.abs(jac[i] - r["J"]).max(),
                    min(np.abs(quat[i] - r["quat"]).max(), np.abs(quat[i] + r["quat"]).max()))
        kr.assert_pose(r, pos[i], quat[i], jac[i], atol=1e-12, what=(name, tool, i))
    print(f"device FK {name} {tool}: worst deviation {worst:.2e}; branches {branches}; {near} of {n} compared up to sign")
    assert near <= 0.02 * n
    if (name, tool) == ("gen4", "rotated"):
        assert min(branches) >= 5, branches


@pytest.mark.parametrize("name,hip_path", [(n, p) for n in ("C2", "C2nd", "C4") for p in ("v2", "v1")], indirect=["hip_path"])
def test_rollout_fx_vs_reference(ctx, name, hip_path):
    """get_fX after solve_recursive(0, ...) -- the rollout of hand-written controls -- on gen7 for PosOrn-1, PosOrn-2 and PosOrnTime-2:
    every step's position and quaternion against the reference evaluated at the device's own X; the velocity entries of the second-order
    state against the oracle's get_fx_jac at the same X; the time entry is the state's.  Non-zero random controls, so that the poses leave
    the start.  The bounds were to be 1e-10 (not the 1e-12 of ilqr_fk_batch, because X itself is read back); the first run on an MI355X
    measured 5.55e-16 at worst on the pose and 2.66e-15 on the velocities (every system and both kernel sets), so they are 100 times
    that: 5.6e-14 and 2.7e-13."""
    Bs = 4
    cfg = dict(workloads.config(name), T=T)
    ch, segs = general_chain("gen7", "rotated")
    desc, inp = workloads.make_batch(ctx, cfg, B=Bs, chain=ch)
    rng = np.random.default_rng(13)
    tm, nd = cfg["kind"] == capi.SYS_POS_ORN_TIME, cfg["nb_deriv"]
    nu = inp["U0"].shape[2]  # a constant part per instance and joint, so that the arm travels, plus a part that changes with the step
    U0 = (rng.uniform(-1.0, 1.0, (Bs, 1, nu)) + 0.3 * rng.uniform(-1.0, 1.0, inp["U0"].shape)) * (0.6 if nd == 1 else 2.0)
    if tm:
        U0[:, :, -1] = rng.uniform(0.15, 0.3, U0.shape[:2])  # dt = u_last^2
    inp = dict(inp, U0=U0)
    p = workloads.load_batch(ctx, desc, inp, Bs)
    p.solve_recursive(0, True, True)
    X, fX = p.X(), p.fX()
    p.close()
    assert np.ptp(X[:, :, :7], axis=1).max() > 0.5  # the joints moved
    ref = _ref_chain("gen7")
    near, worst, worst_v = 0, 0.0, 0.0
    for i in range(Bs):
        s = oracle_system_of_instance(cfg, inp, i, segs) if nd == 2 else None
        for t in range(T):
            r = kr.fk(ref, X[i, t, :7], *_tool("rotated"))
            near += kr.assert_pose(r, fX[i, t, :3], fX[i, t, 3:7], atol=5.6e-14, what=(name, i, t))
            worst = max(worst, np.abs(fX[i, t, :3] - r["pos"]).max(), min(np.abs(fX[i, t, 3:7] - r["quat"]).max(), np.abs(fX[i, t, 3:7] + r["quat"]).max()))
            if nd == 2:
                fo, _ = orc.get_fx_jac(s, X[i, t])
                dv = np.abs(fX[i, t, 7:14] - fo[7:14]).max()
                worst_v = max(worst_v, dv)
                assert dv <= 2.7e-13, (name, i, t, fX[i, t, 7:14], fo[7:14])
            if tm:
                assert fX[i, t, -1] == X[i, t, -1]
    print(f"rollout f(X) {name} [{hip_path}]: pose within {worst:.2e} of the reference, velocities within {worst_v:.2e} of the oracle; "
          f"{near} of {Bs * T} compared up to sign")
    assert near <= 0.02 * Bs * T


# ---- the Riccati solvers


def _gate(ctx, cfg, desc, inp, segs, what):
    p = workloads.load_batch(ctx, desc, inp, B)
    workloads.run_solver(p, cfg, nb_iter=NIT, early_stop=True)
    res = {}

    def oracle_solve(i):
        res[i] = oracle_solve_instance(cfg, inp, i, NIT, True, segs)
        return res[i]

    summ, rel, failures = pp.check_batch(p, cfg, inp, NIT, True, workloads.run_solver, oracle_solve, segs=segs)
    p.close()
    finite = sum(1 for r in res.values() if np.isfinite(r["cost"]))
    print(f"parity {what}: {summ}; oracle finite on {finite} of {B}")
    assert not failures, f"{len(failures)} instance(s) neither within 1e-4 nor proven: {failures[:3]}"
    assert summ["frac_unexplained"] == 0.0
    assert finite >= B // 2  # (the time system's second-order solves diverge on some instances at this horizon, on the Panda too)


@pytest.mark.parametrize("name,hip_path", [(n, p) for n in ("C2", "C3", "C2nd", "C4t1", "C4", "C2ndal") for p in _paths(n)], indirect=["hip_path"])
def test_parity_riccati_gen7(ctx, name, hip_path):
    """Every instance within 1e-4 of the oracle's own end-to-end run or proven iteration by iteration, none unexplained (the gate of
    tests/test_gpu_parity.py), on gen7 with the rotated tool frame.  The AL row is q_6 <= 2.0 as on the Panda."""
    cfg = dict(workloads.config(name), T=T)
    ch, segs = general_chain("gen7", "rotated")
    desc, inp = workloads.make_batch(ctx, cfg, B=B, chain=ch)
    _gate(ctx, cfg, desc, inp, segs, f"{name} gen7 [{hip_path}]")


def _to_frame(Tm, tg):
    """Targets [p, quat, ...] given in the base frame, as seen from the object frame Tm."""
    R, t = Tm[:3, :3], Tm[:3, 3]
    qf = np.array([float(v) for v in kr.eigen_quaternion(kr.mp.matrix(R.T.tolist()))[0]])  # the inverse rotation's quaternion
    out = tg.copy()
    out[:, :3] = (tg[:, :3] - t) @ R
    w, v = tg[:, 3], tg[:, 4:7]
    out[:, 3] = qf[0] * w - v @ qf[1:]
    out[:, 4:7] = qf[0] * v + w[:, None] * qf[1:] + np.cross(qf[1:], v)
    return out


@pytest.mark.parametrize("name,hip_path", [(n, p) for n in ("C2", "C3r") for p in ("v2", "v1")], indirect=["hip_path"])
def test_parity_object_frames_gen7(ctx, name, hip_path):
    """Keypoints seen through object frames on gen7: the via point through a general rotation, the goal through a frame 0.15 rad short of a
    half turn about an oblique axis, where the tool's orientation as seen from the frame leaves the trace branch of Eigen's matrix to
    quaternion rule (tests/test_kinematics_cpu.py counts the branches).  C2 weighs positions only; C3r, the same system with the
    orientation weighted, makes the quaternion's sign count.  Same gate."""
    frames = object_frames()
    cfg = dict(workloads.config(name), T=T, kp_frames=frames)
    ch, segs = general_chain("gen7", "rotated")
    desc, inp = workloads.make_batch(ctx, cfg, B=B, chain=ch)
    for k, Tm in enumerate(frames):
        desc.kp_has_frame[k] = 1
        for a in range(3):
            desc.kp_frame_p[k][a] = Tm[a, 3]
            for b in range(3):
                desc.kp_frame_R[k][a * 3 + b] = Tm[a, b]
    inp = dict(inp, targets=[_to_frame(Tm, tg) for Tm, tg in zip(frames, inp["targets"])])
    _gate(ctx, cfg, desc, inp, segs, f"{name} gen7 object frames [{hip_path}]")


@pytest.mark.parametrize("hip_path", ["v2", "v1", "v2wg"], indirect=True)
def test_parity_narrow_chain_gen4(ctx, hip_path):
    """C2 on gen4 cut behind its third moving joint (y, x and an oblique axis, two fixed joints folded in between): within 1e-4 of the
    oracle at the native three joints or proven iteration by iteration; and the solve is, bit for bit, the real part of the same problem
    padded to seven joints by hand, whose padded entries stay exactly zero."""
    dof = 3
    cfg = dict(nc.narrow_cfg("C2", dof), T=T)
    ch, segs = general_chain("gen4cut3", "rotated")
    assert ch["dof"] == dof
    desc, inp = workloads.make_batch(ctx, cfg, B=B, chain=ch)
    p = workloads.load_batch(ctx, desc, inp, B)
    workloads.run_solver(p, cfg, nb_iter=NIT, early_stop=True)
    nat = nc.results(p, NIT)
    cost, iters = p.cost(), p.iters()
    ct, at = p.trace(NIT)
    states, unexplained, n_proven = None, [], 0
    for i in range(B):
        r = nc.oracle_solve(cfg, inp, i, segs, NIT, early_stop=True)
        assert np.isfinite(r["cost"]), i
        if pp._rel(cost[i], r["cost"]) <= 1e-4 and i >= 4:  # (the first four are proven whatever their distance)
            continue
        if states is None:
            states = pp.gpu_states(p, cfg, NIT, False, workloads.run_solver)
        why = nc.prove(cfg, inp, i, states, ct, at, iters, nc.oracle_system(cfg, inp, i, segs))
        n_proven += why is None
        if why:
            unexplained.append((i, why))
    p.close()
    print(f"parity C2 gen4 (3 joints) [{hip_path}]: {n_proven} proven, {len(unexplained)} unexplained")
    assert not unexplained, unexplained
    p7 = workloads.load_batch(ctx, nc.widen_desc(desc, nc.pad_chain(ch)), nc.widen_inputs(inp, cfg["kind"], cfg["nb_deriv"], dof), B)
    workloads.run_solver(p7, cfg, nb_iter=NIT, early_stop=True)
    wide = nc.results(p7, NIT)
    p7.close()
    nc.assert_embedded(nat, wide, cfg["kind"], cfg["nb_deriv"], dof)


# ---- the batch solvers


@pytest.mark.parametrize("solver", ["batch_cp", "batch"])
def test_parity_batch_solvers_gen7(ctx, hip_path, solver):
    """solve_batch_cp (unit-step basis, K = 2) and solve_batch on C5 at T = 40 on gen7: the oracle's step sizes exactly, its costs within
    1e-4 (as tests/test_gpu_narrow_chain.py::test_parity_batch_solvers)."""
    Bs, nb_iter = 8, 5
    cfg = dict(workloads.config("C5"), T=40)
    ch, segs = general_chain("gen7", "rotated")
    desc, inp = workloads.make_batch(ctx, cfg, B=Bs, chain=ch)
    psi = workloads.psi_of(cfg["psi"], cfg["T"], 7) if solver == "batch_cp" else None
    p = workloads.load_batch(ctx, desc, inp, Bs)
    if psi is None:
        p.solve_batch(nb_iter, False)
    else:
        p.solve_batch_cp(psi, nb_iter, False)
    ct, at = p.trace(nb_iter)
    p.close()
    for i in range(Bs):
        s = oracle_system_of_instance(cfg, inp, i, segs)
        u0 = inp["U0"][i].reshape(-1)
        r = orc.solve_batch_cp(s, psi, u0, nb_iter, False) if psi is not None else orc.solve_batch(s, u0, nb_iter, False)
        n = r["iters"]
        assert n == nb_iter and np.isfinite(r["trace_cost"]).all()
        assert np.array_equal(at[i, :n], r["trace_alpha"]), (i, at[i, :n], r["trace_alpha"])
        assert np.allclose(ct[i, :n], r["trace_cost"], rtol=1e-4, atol=0), (i, ct[i, :n], r["trace_cost"])


# ---- PyLQR


def test_pylqr_general_robot(ctx, hip_path):
    """KDLRobot on gen7.urdf with the rotated tool frame: get_ee_pos, get_ee_orn and J at three configurations within 1e-12 of the
    reference, and a 5-iteration ILQRRecursive solve that is the C-ABI problem's (as test_pylqr_six_joint_robot)."""
    sys.path.insert(0, os.path.join(ROOT, "ilqr_planner_amd", "pylqr"))
    from PyLQR.sim import KDLRobot
    from PyLQR.solver import ILQRRecursive
    from PyLQR.system import PosOrnKeypoint, PosOrnPlannerSys
    from PyLQR.utils import PythonCallbackMessage

    path, base, tip = GENERAL_CHAINS["gen7"]
    rpy, xyz = TOOL_FRAMES["rotated"]
    rng = np.random.default_rng(17)
    q0, dq0 = list(workloads.Q0_TUT), [0.0] * 7
    rbt = KDLRobot(os.path.join(GOLDEN, "chains", path), base, tip, q0, dq0, rpy, xyz)
    ref = _ref_chain("gen7")
    for q in rng.uniform(-3.1, 3.1, (3, 7)):
        rbt.set_conf(q, np.zeros(7), True)
        r = kr.fk(ref, q, rpy, xyz)
        kr.assert_pose(r, np.asarray(rbt.get_ee_pos()), np.asarray(rbt.get_ee_orn()), np.asarray(rbt.J()), atol=1e-12, what=q)
    rbt.set_conf(np.array(q0), np.zeros(7), True)
    ch, _ = general_chain("gen7", "rotated")
    np.testing.assert_array_equal(np.asarray(rbt.joint_lower_limits()), ch["lower"])
    np.testing.assert_array_equal(np.asarray(rbt.joint_upper_limits()), ch["upper"])
    # two keypoints at reachable poses (FK of random configurations), orientation weighted
    Tn, dt, nb_iter = 30, 0.1, 5
    kps_t, Qd = [Tn // 2 - 1, Tn - 1], [1, 1, 1, .1, .1, .1]
    tg = []
    for q in rng.uniform(ch["lower"], ch["upper"], (2, 7)):
        r = kr.fk(ref, q, rpy, xyz)
        tg.append(np.concatenate([r["pos"], r["quat"]]))
    kps = [PosOrnKeypoint(t[:3], t[3:], np.diag(Qd), ts) for t, ts in zip(tg, kps_t)]
    qMax = np.full(7, 10 * np.pi)
    R = [1e-5] * 7
    sys_ = PosOrnPlannerSys(rbt, kps, R, qMax, -qMax, Tn, 1, dt)
    u0 = np.zeros((Tn - 1, 7))
    X, F_X, U, K, k_, cost = ILQRRecursive(sys_).solve(u0, nb_iter, True, True, PythonCallbackMessage())
    desc = capi.make_desc(kind=capi.SYS_POS_ORN, nb_deriv=1, horizon=Tn, dt=dt, R_diag=R, chain=ch, kp_timesteps=kps_t, kp_Q=[np.diag(Qd)] * 2,
                          limits=dict(state_max=qMax, state_min=-qMax, limit_weight=np.ones(7, dtype=int), penalty=1.0))
    p = capi.BatchProblem(ctx, desc, 1)
    p.set_init_state(np.array([q0]), np.array([dq0]))
    for k, t in enumerate(tg):
        p.set_keypoint_targets(k, t[None])
    p.set_controls(u0[None])
    p.solve_recursive(nb_iter, True, True)
    assert np.allclose(np.asarray(X), p.X()[0], rtol=1e-12, atol=1e-14) and np.allclose(cost, p.cost()[0], rtol=1e-12, atol=0)
    assert np.isfinite(cost) and np.abs(np.asarray(X) - np.asarray(X)[0]).max() > 0.1  # a solve that moved
    p.close()
