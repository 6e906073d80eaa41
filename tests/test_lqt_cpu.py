"""Linear-quadratic tracking without a GPU: the NumPy restatement (tests/lqt_reference.py) on known answers, and the parts of
PyLQR.solver.LQT that are checked on the host before any device call (method names, get_nb_states, the "first" errors, IndexError)."""
import os
import sys

import numpy as np
import pytest

from tests import lqt_reference as ref
from tests.helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "ilqr_planner_amd", "pylqr"))


@pytest.fixture(scope="module")
def PyLQR():
    try:
        import PyLQR as m
    except ImportError:
        import __graft_entry__ as g

        g.build()
        import PyLQR as m
    return m


# ---- the restatement

def test_scalar_closed_form():
    # n = m = 1, N = 2, A = B = 1: x_1 = mu_0 + u, minimise Q_1 (x_1 - mu_1)^2 + r u^2
    q0, q1, mu0, mu1, r = 2.0, 3.0, 0.25, -1.5, ref.r_of(0.1, 2)
    want = q1 * (mu1 - mu0) / (q1 + r)
    A, B, Qs, mu = np.eye(1), np.eye(1), [np.array([[q0]]), np.array([[q1]])], np.array([mu0, mu1])
    for u, _ in (ref.linal_dense(A, B, Qs, mu, r), ref.linal_riccati(A, B, Qs, mu, r)):
        assert abs(u[0, 0] - want) <= 1e-15 * abs(want)
    P, d = ref.dp(A, B, Qs, mu, r)
    assert abs(ref.command(A, B, P, d, mu, r, 0, [mu0])[0] - want) <= 1e-15 * abs(want)


def test_r_uses_float_rounding():
    assert ref.r_of(0.1, 2) == float(np.float32(0.1)) ** 2
    assert ref.r_of(0.1, 2) != 0.01 and abs(ref.r_of(0.1, 2) - 0.01) < 1e-9


@pytest.mark.parametrize("n,m,N,seed", [(1, 1, 5, 0), (4, 2, 12, 1), (6, 3, 9, 2), (14, 7, 10, 3), (16, 8, 6, 4)])
def test_linal_forms_agree_and_are_stationary(n, m, N, seed):
    A, B, Qs, mu, r = ref.random_problem(np.random.default_rng(seed), n, m, N)
    ud, xd = ref.linal_dense(A, B, Qs, mu, r)
    ur, xr = ref.linal_riccati(A, B, Qs, mu, r)
    scale = max(np.abs(ud).max(), 1.0)
    assert np.abs(ud - ur).max() <= 1e-10 * scale
    assert np.abs(xd - xr).max() <= 1e-10 * max(np.abs(xd).max(), 1.0)
    g = ref.linal_gradient(A, B, Qs, mu, r, ud)
    assert np.abs(g).max() <= 1e-9 * scale * max(np.abs(Qs).max(), 1.0) * N


@pytest.mark.parametrize("n,m,seed", [(4, 2, 5), (14, 7, 6)])
def test_reference_command_is_the_optimal_law(n, m, seed):
    # the reference's command at tau = t + 1 uses mu_tau in both places; the terms cancel to the optimal law L (mu_tau - A x) - H d_tau,
    # so closing the loop from x_0 = mu_0 reproduces the LinAl minimiser
    A, B, Qs, mu, r = ref.random_problem(np.random.default_rng(seed), n, m, 11)
    ur, xr = ref.linal_riccati(A, B, Qs, mu, r)
    P, d = ref.dp(A, B, Qs, mu, r)
    for t in range(10):
        np.testing.assert_allclose(ref.command(A, B, P, d, mu, r, t, xr[t]), ur[t], rtol=0, atol=1e-11 * np.abs(ur).max())


# ---- PyLQR.solver.LQT on the host

def _lqt(PyLQR, N=5, nq=None):
    A, B = ref.double_integrator(2, 0.1)
    Qs = [np.eye(4)] * (nq if nq is not None else N)
    return PyLQR.solver.LQT(A, B, Qs, np.zeros(4 * N + 3), 0.1, 2)  # 3 trailing entries: N = size / n (integer division)


def test_pylqr_lqt_surface(PyLQR):
    from PyLQR.solver import LQT

    for name in ("solve_DP", "solve_lin_al", "get_nb_states", "get_predicted_states", "get_command"):
        assert hasattr(LQT, name), name
    with pytest.raises(TypeError):  # positional only, as the reference binds it
        LQT(A=np.eye(2), B=np.ones((2, 1)), Qs=[np.eye(2)], states=np.zeros(2), rfactor=0.1, nb_deriv=2)
    with pytest.raises(TypeError):  # no defaults
        LQT(np.eye(2), np.ones((2, 1)), [np.eye(2)], np.zeros(2))


def test_pylqr_lqt_host_checks(PyLQR):
    lqt = _lqt(PyLQR, N=5)
    assert lqt.get_nb_states() == 5
    with pytest.raises(RuntimeError, match=r"^solveLinal\(\) or solveQP\(\) first$"):
        lqt.get_command(0)
    with pytest.raises(RuntimeError, match=r"^solveLinal\(\) or solveQP\(\) first$"):
        lqt.get_predicted_states()
    with pytest.raises(RuntimeError, match=r"^solveDP\(\) first$"):
        lqt.get_command(0, np.zeros(4))
    # too few precisions: the reference's Qs.at throws std::out_of_range before anything is solved
    short = _lqt(PyLQR, N=5, nq=3)
    with pytest.raises(IndexError):
        short.solve_DP()
    with pytest.raises(IndexError):
        _lqt(PyLQR, N=5, nq=4).solve_lin_al()
    with pytest.raises(IndexError):
        _lqt(PyLQR, N=5, nq=0).solve_DP()
