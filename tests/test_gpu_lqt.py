"""Linear-quadratic tracking on the device (ilqr_planner_amd/csrc/ilqr_lqt.hip): PyLQR.solver.LQT and capi.LQTBatch against the NumPy
restatement (tests/lqt_reference.py), batch-size independence, shared vs per-instance precisions, device pointers, error texts."""
import os
import sys

import numpy as np
import pytest

from ilqr_planner_amd import capi
from tests import lqt_reference as ref
from tests.helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "ilqr_planner_amd", "pylqr"))

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (4, 2), (6, 3), (14, 7), (16, 8)]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def PyLQR():
    import PyLQR as m

    return m


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _batch_problem(n, m, N, B, per_instance, seed):
    rng = np.random.default_rng(seed)
    A, Bm, Qs, _, r = ref.random_problem(rng, n, m, N)
    if per_instance:
        Qs = np.array([ref.random_problem(rng, n, m, N)[2] for _ in range(min(B, 4))])
        Qs = Qs[np.arange(B) % len(Qs)]
    mu = rng.standard_normal((B, N, n))
    return A, Bm, Qs, mu, r


def _check_instance(lq, A, Bm, Qs_i, mu_i, r, b, P_all, d_all, U_all, X_all, xs, us_all, ts):
    P, d = ref.dp(A, Bm, Qs_i, mu_i.reshape(-1), r)
    assert _rel(P_all, P) <= 1e-9 and _rel(d_all[b], d) <= 1e-9
    ud, xd = ref.linal_dense(A, Bm, Qs_i, mu_i.reshape(-1), r)
    ur, xr = ref.linal_riccati(A, Bm, Qs_i, mu_i.reshape(-1), r)
    su, sx = max(np.abs(ud).max(), 1.0), max(np.abs(xd).max(), 1.0)
    assert np.abs(U_all[b] - ud).max() <= np.abs(ur - ud).max() + 1e-9 * su
    assert np.abs(X_all[b] - xd).max() <= np.abs(xr - xd).max() + 1e-9 * sx
    for t, us in zip(ts, us_all):
        want = ref.command(A, Bm, P, d, mu_i.reshape(-1), r, t, xs[b])
        assert np.abs(us[b] - want).max() <= 1e-9 * max(np.abs(want).max(), 1.0)


@pytest.mark.parametrize("per_instance", [False, True])
@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("B", [1, 7, 256, 4096])
def test_batch_matches_restatement(ctx, n, m, B, per_instance):
    N = 12
    A, Bm, Qs, mu, r = _batch_problem(n, m, N, B, per_instance, seed=n * 100 + m + B)
    lq = capi.LQTBatch(ctx, A, Bm, Qs, mu, r, qs_per_instance=per_instance)
    lq.solve_dp()
    P_all, d_all = lq.P(), lq.d()
    rng = np.random.default_rng(B)
    xs = rng.standard_normal((B, n))
    ts = (-1, 0, N // 2, N - 2)
    us_all = [lq.command(t, xs) for t in ts]
    lq.solve_lin_al()
    U_all, X_all = lq.U(), lq.X()
    assert np.all(np.isfinite(U_all)) and np.all(np.isfinite(X_all))
    for b in sorted({0, B // 2, B - 1, min(3, B - 1)}):
        _check_instance(lq, A, Bm, Qs[b] if per_instance else Qs, mu[b], r, b, P_all[b] if per_instance else P_all, d_all, U_all, X_all, xs,
                        us_all, ts)
    lq.close()


@pytest.mark.parametrize("per_instance", [False, True])
@pytest.mark.parametrize("n,m", [(4, 2), (14, 7)])
def test_batch_cut_out_is_bit_identical(ctx, n, m, per_instance):
    N, B, lo, hi = 20, 300, 100, 107
    A, Bm, Qs, mu, r = _batch_problem(n, m, N, B, per_instance, seed=7)
    x = np.random.default_rng(1).standard_normal((B, n))
    outs = []
    for sl in (slice(0, B), slice(lo, hi)):
        lq = capi.LQTBatch(ctx, A, Bm, Qs[sl] if per_instance else Qs, mu[sl], r, qs_per_instance=per_instance)
        lq.solve_lin_al()
        outs.append((lq.U(), lq.X(), lq.d(), lq.command(3, x[sl]), lq.P()))
        lq.close()
    big, small = outs
    for k in range(4):
        assert np.array_equal(big[k][lo:hi], small[k])
    assert np.array_equal(big[4][lo:hi] if per_instance else big[4], small[4])


@pytest.mark.parametrize("n,m", [(4, 2), (14, 7)])
def test_equal_per_instance_precisions_match_shared(ctx, n, m):
    N, B = 30, 64
    A, Bm, Qs, mu, r = _batch_problem(n, m, N, B, False, seed=11)
    x = np.random.default_rng(2).standard_normal((B, n))
    res = []
    for per in (False, True):
        lq = capi.LQTBatch(ctx, A, Bm, np.broadcast_to(Qs, (B,) + Qs.shape) if per else Qs, mu, r, qs_per_instance=per)
        lq.solve_lin_al()
        res.append((lq.U(), lq.X(), lq.d(), lq.command(0, x), lq.P()[0] if per else lq.P()))
        lq.close()
    for a, b in zip(*res):
        assert _rel(a, b) <= 1e-12


def test_dev_variants_bit_identical():
    """In a fresh process that initialises torch's device first (as bench.py does): tests/tools/lqt_dev.py."""
    import subprocess

    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "lqt_dev.py")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "lqt dev variants: ok"


def test_errors(ctx):
    A, Bm, Qs, mu, r = _batch_problem(4, 2, 5, 3, False, seed=5)
    with pytest.raises(RuntimeError, match=r"n_x must be in 1\.\.16 \(got 17\)"):
        capi.LQTBatch(ctx, np.eye(17), np.ones((17, 2)), np.broadcast_to(np.eye(17), (5, 17, 17)), np.zeros((3, 5, 17)), r)
    with pytest.raises(RuntimeError, match=r"n_u must be in 1\.\.8 \(got 9\)"):
        capi.LQTBatch(ctx, A, np.ones((4, 9)), Qs, mu, r)
    with pytest.raises(RuntimeError, match=r"N must be >= 1 \(got 0\)"):
        capi.LQTBatch(ctx, A, Bm, Qs[:0], mu[:, :0], r)
    lq = capi.LQTBatch(ctx, A, Bm, Qs, mu, r)
    with pytest.raises(RuntimeError, match=r"^solveDP\(\) first$"):
        lq.command(0, np.zeros((3, 4)))
    with pytest.raises(RuntimeError, match=r"^solveLinal\(\) or solveQP\(\) first$"):
        lq.U()
    lq.solve_dp()
    for t in (-2, 4):
        with pytest.raises(RuntimeError, match=rf"t must be in -1\.\.3 \(got {t}\)"):
            lq.command(t, np.zeros((3, 4)))
    lq.close()


def test_nonfinite_inputs_give_nonfinite_outputs(ctx):
    A, Bm = ref.double_integrator(2, 0.1)
    N = 8
    Qs = np.zeros((N, 4, 4))  # B'PB singular and r = 0: S = 0
    lq = capi.LQTBatch(ctx, A, Bm, Qs, np.ones((5, N, 4)), 0.0)
    lq.solve_lin_al()
    assert not np.all(np.isfinite(lq.U()))
    lq.close()
    lq = capi.LQTBatch(ctx, A, Bm, np.broadcast_to(np.eye(4), (N, 4, 4)), np.full((5, N, 4), np.nan), 0.1)
    lq.solve_lin_al()
    assert np.all(np.isnan(lq.X()))
    lq.close()


# ---- PyLQR.solver.LQT

def _via_points(N=40):
    A, B = ref.double_integrator(2, 0.05)
    Qs = [np.zeros((4, 4)) for _ in range(N)]
    mu = np.zeros((N, 4))
    for t, p in ((N // 3, (1.0, 0.5)), (2 * N // 3, (-0.5, 1.5)), (N - 1, (0.2, -0.3))):
        Qs[t] = np.diag([1.0, 1.0, 0.0, 0.0]) * 1e2
        mu[t, :2] = p
    Qs[-1] = np.eye(4) * 1e2  # stop at the last via-point
    return A, B, Qs, mu.reshape(-1)


def test_pylqr_via_points(PyLQR):
    A, B, Qs, mu = _via_points()
    N, r = 40, ref.r_of(0.1, 2)
    lqt = PyLQR.solver.LQT(A, B, Qs, mu, 0.1, 2)
    assert lqt.get_nb_states() == N
    lqt.solve_DP()
    P, d = ref.dp(A, B, Qs, mu, r)
    x, xr = mu[:4].copy(), mu[:4].copy()
    for t in range(-1, N - 1):  # closed loop with the reference's law; the same states on both sides
        u = lqt.get_command(t, x)
        want = ref.command(A, B, P, d, mu, r, t, x)
        assert np.abs(u - want).max() <= 1e-9 * max(np.abs(want).max(), 1.0)
        x = A @ x + B @ want
    lqt.solve_lin_al()
    ud, xd = ref.linal_dense(A, B, Qs, mu, r)
    ur, _ = ref.linal_riccati(A, B, Qs, mu, r)
    tol = np.abs(ur - ud).max() + 1e-9 * np.abs(ud).max()
    for t in range(N - 1):
        assert np.abs(lqt.get_command(t) - ud[t]).max() <= tol
    xs = lqt.get_predicted_states()
    assert xs.shape == (N * 4,)
    assert np.abs(xs - xd.reshape(-1)).max() <= tol * N
    assert np.array_equal(xs[:4], mu[:4])
    with pytest.raises(IndexError):
        lqt.get_command(N - 1, x)
    with pytest.raises(IndexError):
        lqt.get_command(-2, x)
    with pytest.raises(IndexError):
        lqt.get_command(N - 1)


def test_pylqr_scalar_closed_form_uses_float_r(PyLQR):
    q0, q1, mu0, mu1 = 2.0, 3.0, 0.25, -1.5
    lqt = PyLQR.solver.LQT(np.eye(1), np.eye(1), [np.array([[q0]]), np.array([[q1]])], np.array([mu0, mu1]), 0.1, 2)
    lqt.solve_lin_al()
    u = lqt.get_command(0)[0]
    want = q1 * (mu1 - mu0) / (q1 + ref.r_of(0.1, 2))
    with_r001 = q1 * (mu1 - mu0) / (q1 + 0.01)
    assert abs(u - want) <= 1e-14 * abs(want)
    assert abs(u - with_r001) > 1e-12 * abs(want)  # r = 0.010000000298..., not 0.01: a 1e-10 relative shift


def test_pylqr_more_precisions_than_states(PyLQR):
    rng = np.random.default_rng(9)
    N = 10
    A, B, Qs, mu, _ = ref.random_problem(rng, 4, 2, N, Qs_count=N + 2)
    r = ref.r_of(0.1, 2)
    lqt = PyLQR.solver.LQT(A, B, list(Qs), mu, 0.1, 2)
    lqt.solve_DP()
    x = rng.standard_normal(4)
    P_back, d_back = ref.dp(A, B, Qs[:N - 1], mu, r, q_last=Qs[-1])  # DP: Qs.back() at N-1
    P_n1, d_n1 = ref.dp(A, B, Qs[:N], mu, r)
    u = lqt.get_command(N - 3, x)
    want = ref.command(A, B, P_back, d_back, mu, r, N - 3, x)
    other = ref.command(A, B, P_n1, d_n1, mu, r, N - 3, x)
    assert np.abs(u - want).max() <= 1e-9 * np.abs(want).max() < np.abs(other - want).max()
    lqt.solve_lin_al()  # LinAl: Qs[0 .. N-1]
    ud, _ = ref.linal_dense(A, B, Qs[:N], mu, r)
    ur, _ = ref.linal_riccati(A, B, Qs[:N], mu, r)
    got = np.array([lqt.get_command(t) for t in range(N - 1)])
    assert np.abs(got - ud).max() <= np.abs(ur - ud).max() + 1e-9 * np.abs(ud).max()
