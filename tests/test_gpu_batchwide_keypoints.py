"""BatchILQR and wide-basis BatchILQRCP with many keypoints: m = n_kp n_x above 32 keypoint rows, up to ILQR_MAX_KP n_x (the kernels of
ilqr_batchwide_big.hip), against the oracle's dense restatement of the reference (BatchILQR.cpp:110-173, BatchILQRCP.cpp:109-175) through
the parity gate of test_gpu_batchwide.py.  Every case here has more than 32 keypoint rows."""
import os
import re
import sys

import numpy as np
import pytest

from tests import parity_proof as pp
from tests.helpers import GOLDEN, ROOT, oracle_system_of_instance, orc

pytestmark = pytest.mark.gpu

NX = {"C2": 7, "C2nd": 14, "C1": 7, "C1j": 7, "C4t1": 8, "C4": 15, "C1t": 8}  # device n_x (joint chains are padded to 7 joints)


@pytest.fixture(scope="module")
def ctx():
    from ilqr_planner_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


def _cfg(name, T, kp_t):
    """workload `name` at horizon T with keypoints at kp_t: via points weighted like its via point, the last like its goal; continuous
    times of the time systems spread up to its goal's."""
    from ilqr_planner_amd import workloads

    cfg = dict(workloads.config(name), T=T)
    n = len(kp_t)
    cfg["Qdiag"] = [cfg["Qdiag"][0]] * (n - 1) + [cfg["Qdiag"][1]]
    if cfg.get("ctimes"):
        cfg["ctimes"] = [cfg["ctimes"][1] * (k + 1) / n for k in range(n)]
    return cfg


def _first_step_sensitivity(cfg, inp, i, s, psi, ref):
    """Largest relative move of the oracle's cost after one step over its neutral arithmetic variants and one-ulp perturbations of the
    initial controls (tests/parity_proof.py: what a backward-stable solve may differ by).  With m ~ 50 .. 120 keypoint rows the normal
    matrix J'QJ ~ 1 against R = 1e-5 is conditioned so that rounding alone moves this cost by ~1e-10."""
    u0 = pp._u_oracle(cfg, inp, inp["U0"][i])

    def run(pt=None):
        u = u0 if pt is None else u0 * (1.0 + np.where(np.arange(u0.size) % 2 == 0, pt[0], pt[1]) * 2.0 ** -52)
        return orc.solve_batch(s, u, 2, False) if psi is None else orc.solve_batch_cp(s, psi, u, 2, False)

    return pp._variant_sensitivity(run, lambda rv: rv["trace_cost"][1], ref, run)


def _compare(p, cfg, inp, B, nb_iter, psi, tol=1e-6, step_tol=1e-10):
    """The gate of test_gpu_batchwide._compare (every instance within `tol` of the oracle's run with its step sizes, or proven iteration
    by iteration; none excused), on the true number of joints of narrow joint-space chains."""
    U, X = pp._unpad(cfg, inp, p.U()), pp._unpad(cfg, inp, p.X())
    ct, at = p.trace(nb_iter)
    cost = p.cost()
    solve = (lambda q, n, es: q.solve_batch(n, es)) if psi is None else (lambda q, n, es: q.solve_batch_cp(psi, n, es))
    summ, rel, failures, runs = pp.check_batch_solver(p, cfg, inp, psi, nb_iter, False, solve, rtol=tol)
    print(f"parity {summ}")
    assert not failures, f"{len(failures)} instance(s) neither within {tol} nor proven: {failures[:3]}"
    for i in range(B):
        r = runs[i]
        s = oracle_system_of_instance(cfg, inp, i)
        if rel[i] <= tol:
            rl = np.abs(ct[i] - r["trace_cost"]) / np.maximum(np.abs(r["trace_cost"]), 1e-12)
            if rl[1] > step_tol:  # one step is rounding only; past step_tol only within the oracle's own sensitivity at that step
                sens = _first_step_sensitivity(cfg, inp, i, s, psi, r["trace_cost"][1])
                print(f"instance {i}: first step {rl[1]:.2e}, oracle sensitivity {sens:.2e}")
                assert rl[1] <= pp.ILL_FACTOR * sens, f"instance {i}: cost after the first step differs by {rl[1]:.2e} (oracle sensitivity {sens:.2e})"
            np.testing.assert_allclose(U[i].reshape(-1), r["u"], rtol=0, atol=tol * max(1.0, np.abs(r["u"]).max()))
        x = np.asarray(X[i][0])
        for k in range(cfg["T"] - 1):
            x = orc.step(s, x, U[i][k])[0]
        np.testing.assert_allclose(X[i][-1], x, rtol=0, atol=1e-9 * max(1.0, np.abs(x).max()))
        assert np.isfinite(cost[i])


def _spread(T, n):
    return [int(round((k + 1) * (T - 1) / n)) for k in range(n)]


def _batch(ctx, name, T, kp_t, B, limits="inactive", u0_scale=0.0, seed=3):
    from ilqr_planner_amd import workloads

    cfg = _cfg(name, T, kp_t)
    desc, inp = workloads.make_batch(ctx, cfg, B=B, limits=limits, kp_t=kp_t)
    if u0_scale:
        noise = u0_scale * np.random.default_rng(seed).standard_normal(inp["U0"].shape)
        if cfg["kind"] in (2, 3):  # the joints a narrow chain is padded with stay at rest (the oracle has none)
            noise[..., inp.get("dof", 7):7] = 0.0
        inp["U0"] = inp["U0"] + noise
    return cfg, desc, inp


CASES = [("C2", 30, 5, "inactive", 0.0), ("C2", 32, 8, "urdf", 0.3), ("C2nd", 24, 3, "inactive", 0.5), ("C2nd", 24, 8, "urdf", 0.0),
         ("C1", 30, 6, "urdf", 0.2), ("C4t1", 24, 5, "urdf", 0.02), ("C4t1", 24, 8, "inactive", 0.02), ("C4", 20, 3, "inactive", 0.02),
         ("C4", 20, 8, "urdf", 0.02), ("C1t", 20, 5, "inactive", 0.01)]


@pytest.mark.parametrize("name,T,n_kp,limits,u0_scale", CASES, ids=[f"{c[0]}-kp{c[2]}-m{c[2] * NX[c[0]]}" for c in CASES])
def test_batch_ilqr_many_keypoints_vs_oracle(ctx, name, T, n_kp, limits, u0_scale):
    """BatchILQR on every system shape past 32 keypoint rows and at the top of the range (PosOrn-1 m = 56, PosOrn-2 m = 112, PosOrnTime-1
    m = 64, PosOrnTime-2 m = 120), zero and random initial controls, inactive and URDF limits.  Tolerances of test_gpu_batchwide.py: one
    step to rounding (1e-10) and the trace to 1e-6 on the constant-dt systems, 1e-4 on the time systems."""
    from ilqr_planner_amd import workloads

    assert n_kp * NX[name] > 32
    B, nb_iter = 8, 5
    cfg, desc, inp = _batch(ctx, name, T, _spread(T, n_kp), B, limits, u0_scale)
    p = workloads.load_batch(ctx, desc, inp, B)
    p.solve_batch(nb_iter, False)
    _compare(p, cfg, inp, B, nb_iter, None, tol=1e-4 if cfg["kind"] in (1, 3) else 1e-6)
    p.close()


@pytest.mark.parametrize("name,T,n_kp,basis,K,u0_scale", [("C2", 40, 6, "rbf", 5, 0.0), ("C2", 30, 8, "bernstein", 4, 0.3), ("C2nd", 24, 4, "sawtooth", 3, 0.4),
                                                          ("C2nd", 24, 8, "rbf", 4, 0.0)])
def test_wide_basis_cp_many_keypoints_vs_oracle(ctx, name, T, n_kp, basis, K, u0_scale):
    """BatchILQRCP with Kw = 7 K > 16 (overlapping bases) past 32 keypoint rows; the tolerances of test_wide_basis_cp_vs_oracle (the
    overlapping bases make H ill-conditioned: 1e-4 on the trace, 1e-8 on the first step)."""
    from ilqr_planner_amd import workloads

    assert n_kp * NX[name] > 32
    B, nb_iter = 8, 5
    cfg, desc, inp = _batch(ctx, name, T, _spread(T, n_kp), B, "urdf", u0_scale, seed=4)
    p = workloads.load_batch(ctx, desc, inp, B)
    psi = np.kron(orc.psi(basis, T - 1, K), np.eye(7))
    assert psi.shape[1] > 16
    p.solve_batch_cp(psi, nb_iter, False)
    _compare(p, cfg, inp, B, nb_iter, psi, tol=1e-4, step_tol=1e-8)
    p.close()


@pytest.mark.parametrize("name,n_kp", [("C2", 6), ("C2nd", 8)])
def test_wide_equals_narrow_path_many_keypoints(ctx, name, n_kp):
    """The identity basis as an explicit matrix (Cholesky inverse of PSI'R PSI, projection of u0) and the built-in identity take the two
    routes of the m > 32 kernels; they agree to rounding."""
    from ilqr_planner_amd import workloads

    B, nb_iter, T = 6, 4, 12
    cfg, desc, inp = _batch(ctx, name, T, _spread(T, n_kp), B, u0_scale=0.2)
    p = workloads.load_batch(ctx, desc, inp, B)
    p.solve_batch(nb_iter, False)
    U1, c1 = p.U(), p.trace(nb_iter)[0]
    p.set_controls(inp["U0"])
    p.solve_batch_cp(np.eye((T - 1) * 7), nb_iter, False)
    U2, c2 = p.U(), p.trace(nb_iter)[0]
    np.testing.assert_allclose(c1, c2, rtol=1e-9)
    np.testing.assert_allclose(U1, U2, rtol=0, atol=1e-8 * max(1.0, np.abs(U1).max()))
    p.close()


EDGES = [("C2", 9, [0, 1, 2, 5, 8], 67), ("C2nd", 12, [8, 9, 10, 11], 1), ("C2", 65, [10, 20, 30, 40, 64], 13), ("C2nd", 66, [16, 32, 48, 65], 7),
         ("C4t1", 10, [0, 1, 2, 3, 9], 5), ("C4", 12, [1, 2, 11], 3), ("C1", 8, [1, 2, 3, 4, 5, 6, 7], 4)]


@pytest.mark.parametrize("name,T,kp_t,B", EDGES, ids=[f"{e[0]}-T{e[1]}-kp{'_'.join(map(str, e[2]))}-B{e[3]}" for e in EDGES])
def test_batch_ilqr_many_keypoints_edge_shapes(ctx, name, T, kp_t, B):
    """Keypoints on steps 0 and 1 (the reference's shifted sensitivity is empty there), on consecutive steps and on the last step, a single
    instance and a batch of 67, T = 65 and 66, early stop on: BatchILQR against the oracle."""
    from ilqr_planner_amd import workloads

    nb_iter = 4
    cfg, desc, inp = _batch(ctx, name, T, kp_t, B, u0_scale=0.02 if name.startswith("C4") else 0.1)
    assert len(kp_t) * NX[name] > 32
    p = workloads.load_batch(ctx, desc, inp, B)
    p.solve_batch(nb_iter, True)
    ct, at = p.trace(nb_iter)
    iters, U = p.iters(), p.U()
    p.close()
    for i in sorted(set([0, B // 2, B - 1])):
        s = oracle_system_of_instance(cfg, inp, i)
        r = orc.solve_batch(s, pp._u_oracle(cfg, inp, inp["U0"][i]), nb_iter, True)
        n = r["iters"]
        assert iters[i] == n
        np.testing.assert_array_equal(at[i][:n], r["trace_alpha"])
        tol = 1e-4 if cfg["kind"] in (1, 3) else 1e-6
        np.testing.assert_allclose(ct[i][:min(n, 2)], r["trace_cost"][:2], rtol=1e-9)
        np.testing.assert_allclose(ct[i][:n], r["trace_cost"], rtol=tol)
        assert np.all(np.isnan(ct[i][n:]))
        np.testing.assert_allclose(pp._u_oracle(cfg, inp, U[i]), r["u"], rtol=0, atol=tol * max(1.0, np.abs(r["u"]).max()))


@pytest.mark.parametrize("name,n_kp", [("C2nd", 8), ("C4", 8)])
def test_cut_out_is_bit_identical(ctx, name, n_kp):
    """3 instances cut out of a 300-instance batch give the same bits of cost, U and X as in the whole batch."""
    from ilqr_planner_amd import workloads

    B, T, nb_iter, pick = 300, 20, 4, [0, 151, 299]
    cfg, desc, inp = _batch(ctx, name, T, _spread(T, n_kp), B, "urdf", 0.02)
    p = workloads.load_batch(ctx, desc, inp, B)
    p.solve_batch(nb_iter, False)
    full = (p.cost(), p.U(), p.X(), p.trace(nb_iter)[0])
    p.close()
    sub = dict(inp, q0=inp["q0"][pick], dq0=inp["dq0"][pick], U0=inp["U0"][pick], targets=[t[pick] for t in inp["targets"]])
    q = workloads.load_batch(ctx, desc, sub, len(pick))
    q.solve_batch(nb_iter, False)
    part = (q.cost(), q.U(), q.X(), q.trace(nb_iter)[0])
    q.close()
    for a, b in zip(full, part):
        np.testing.assert_array_equal(np.asarray(a)[pick], np.asarray(b))


LINE = re.compile(r"Iteration (\d+), Cost: (\S+), alpha= ([^,\s]+)")


def test_pylqr_batch_solvers_six_keypoints(ctx, capsys):
    """PyLQR's BatchILQR(sys) and BatchILQRCP(sys, PSI) on a PosOrnPlannerSys with 6 keypoints (m = 42) reach the device's m > 32 kernels:
    the oracle's step sizes, the printed cost trace and the controls."""
    sys.path.insert(0, os.path.join(ROOT, "ilqr_planner_amd", "pylqr"))
    from PyLQR.sim import KDLRobot
    from PyLQR.solver import BatchILQR, BatchILQRCP
    from PyLQR.system import PosOrnKeypoint, PosOrnPlannerSys
    from PyLQR.utils import PythonCallbackMessage

    T, nb_iter, kp_t = 40, 6, [6, 12, 19, 26, 32, 39]
    cfg, desc, inp = _batch(ctx, "C2", T, kp_t, 1)
    q0 = inp["q0"][0]
    qMax = np.array([np.pi] * 7) * 10
    rbt = KDLRobot(os.path.join(GOLDEN, "panda_chain.urdf"), "panda_link0", "panda_tip", q0.tolist(), [0.0] * 7)
    kps = [PosOrnKeypoint(inp["targets"][k][0][0:3], inp["targets"][k][0][3:7], np.diag(cfg["Qdiag"][k]), t) for k, t in enumerate(kp_t)]
    sys_ = PosOrnPlannerSys(rbt, kps, [1e-5] * 7, qMax, -qMax, T, 1, cfg["dt"])
    s = oracle_system_of_instance(cfg, inp, 0)
    u0 = np.zeros((T - 1) * 7)
    psi = np.kron(orc.psi("rbf", T - 1, 5), np.eye(7))
    for planner, r in [(BatchILQR(sys_), orc.solve_batch(s, u0, nb_iter, False)), (BatchILQRCP(sys_, psi), orc.solve_batch_cp(s, psi, u0, nb_iter, False))]:
        capsys.readouterr()
        U = np.asarray(planner.solve(nb_iter, u0, False, PythonCallbackMessage())).reshape(-1)
        lines = capsys.readouterr().out.strip().splitlines()
        assert len(lines) == nb_iter
        for it, ln in enumerate(lines):
            mt = LINE.match(ln)
            assert mt and int(mt.group(1)) == it + 1, ln
            assert float(mt.group(3)) == r["trace_alpha"][it], ln
            assert abs(float(mt.group(2)) - r["trace_cost"][it]) <= 1e-5 * abs(r["trace_cost"][it]), ln  # printed to 6 significant digits
        np.testing.assert_allclose(U, r["u"], rtol=0, atol=1e-4 * max(1.0, np.abs(r["u"]).max()))
