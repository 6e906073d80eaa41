"""NumPy restatement of linear-quadratic tracking (solver::LQT), written from its equations: x' = A x + B u, targets mu_t (t = 0..N-1), cost
sum_t (x_t - mu_t)' Q_t (x_t - mu_t) + sum_t u_t' R u_t with R = r I.  Used by tests/test_lqt_cpu.py and tests/test_gpu_lqt.py.

- dp:            P_{N-1} = Q_last, d_{N-1} = 0;  S = B'P'B + R,  P_t = Q_t - A'(P' B S^-1 B' P' - P') A,
                 d_t = (A' - A' P' B S^-1 B')(P' (A mu_t - mu_{t+1}) + d') with P' = P_{t+1}, d' = d_{t+1}.
- command:       the DP command at tau = t + 1 with the reference's convention: K = S^-1 B' P_tau A, f = -S^-1 B' (P_tau (A mu_tau - mu_tau) + d_tau),
                 u = K (mu_tau - x) + f.
- linal_dense:   u = (Su' Q Su + R)^-1 Su' Q (mu - Sx mu_0), x = Su u + Sx mu_0 (the normal equations, formed densely).
- linal_riccati: the same minimiser from the DP recursion (terminal weight Q_{N-1}) and a rollout from x_0 = mu_0 with the optimal law
                 u_t = -S^-1 B' (P_{t+1} (A x_t - mu_{t+1}) + d_{t+1}).
"""
import numpy as np


def r_of(rfactor, nb_deriv):
    """R's diagonal: the constructor's rfactor is a C float, raised to nb_deriv in double."""
    return float(np.float32(rfactor)) ** nb_deriv


def _targets(mu, n):
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    N = mu.size // n
    return mu[: N * n].reshape(N, n), N


def dp(A, B, Qs, mu, r, q_last=None):
    """P[N][n][n], d[N][n]; Qs[t] for t < N-1, q_last (default Qs[-1]) at N-1."""
    A, B = np.asarray(A, float), np.asarray(B, float)
    n, m = A.shape[1], B.shape[1]
    M, N = _targets(mu, n)
    P, d = [None] * N, [None] * N
    P[N - 1] = np.asarray(Qs[-1] if q_last is None else q_last, float)
    d[N - 1] = np.zeros(n)
    R = r * np.eye(m)
    for t in range(N - 2, -1, -1):
        Pn, dn = P[t + 1], d[t + 1]
        Si = np.linalg.inv(B.T @ Pn @ B + R)
        P[t] = np.asarray(Qs[t], float) - A.T @ (Pn @ B @ Si @ B.T @ Pn - Pn) @ A
        d[t] = (A.T - A.T @ Pn @ B @ Si @ B.T) @ (Pn @ (A @ M[t] - M[t + 1]) + dn)
    return np.array(P), np.array(d)


def command(A, B, P, d, mu, r, t, x):
    """getCommand(t, x) with the reference's convention (tau = t + 1, mu_tau in both places)."""
    A, B = np.asarray(A, float), np.asarray(B, float)
    n, m = A.shape[1], B.shape[1]
    M, _ = _targets(mu, n)
    tau = t + 1
    Si = np.linalg.inv(B.T @ P[tau] @ B + r * np.eye(m))
    K = Si @ B.T @ P[tau] @ A
    f = -Si @ B.T @ (P[tau] @ (A @ M[tau] - M[tau]) + d[tau])
    return K @ (M[tau] - np.asarray(x, float)) + f


def linal_dense(A, B, Qs, mu, r):
    """(u [N-1][m], x [N][n]) from the dense normal equations with Q = blkdiag(Qs[0..N-1])."""
    A, B = np.asarray(A, float), np.asarray(B, float)
    n, m = A.shape[1], B.shape[1]
    M, N = _targets(mu, n)
    Su = np.zeros((N * n, (N - 1) * m))
    Sx = np.zeros((N * n, n))
    Q = np.zeros((N * n, N * n))
    Sx[:n] = np.eye(n)
    Q[:n, :n] = Qs[0]
    for i in range(1, N):
        Sx[i * n:(i + 1) * n] = Sx[(i - 1) * n:i * n] @ A
        for j in range(i):  # x_i = A^(i-1-j) B u_j
            Su[i * n:(i + 1) * n, j * m:(j + 1) * m] = np.linalg.matrix_power(A, i - 1 - j) @ B
        Q[i * n:(i + 1) * n, i * n:(i + 1) * n] = Qs[i]
    R = r * np.eye((N - 1) * m)
    mu_f = M.reshape(-1)
    u = np.linalg.inv(Su.T @ Q @ Su + R) @ Su.T @ Q @ (mu_f - Sx @ M[0])
    x = Su @ u + Sx @ M[0]
    return u.reshape(N - 1, m), x.reshape(N, n)


def linal_riccati(A, B, Qs, mu, r):
    """(u [N-1][m], x [N][n]): the DP recursion with terminal weight Qs[N-1], rolled out from x_0 = mu_0 with the optimal law."""
    A, B = np.asarray(A, float), np.asarray(B, float)
    n, m = A.shape[1], B.shape[1]
    M, N = _targets(mu, n)
    P, d = dp(A, B, Qs[:N], mu, r)
    x = np.zeros((N, n))
    u = np.zeros((max(N - 1, 0), m))
    x[0] = M[0]
    for t in range(N - 1):
        Si = np.linalg.inv(B.T @ P[t + 1] @ B + r * np.eye(m))
        u[t] = -Si @ B.T @ (P[t + 1] @ (A @ x[t] - M[t + 1]) + d[t + 1])
        x[t + 1] = A @ x[t] + B @ u[t]
    return u, x


def linal_gradient(A, B, Qs, mu, r, u):
    """Gradient of the tracking cost in the stacked controls u [N-1][m] (x_0 = mu_0)."""
    A, B = np.asarray(A, float), np.asarray(B, float)
    n, m = A.shape[1], B.shape[1]
    M, N = _targets(mu, n)
    x = np.zeros((N, n))
    x[0] = M[0]
    for t in range(N - 1):
        x[t + 1] = A @ x[t] + B @ u[t]
    lam = 2 * np.asarray(Qs[N - 1], float) @ (x[N - 1] - M[N - 1])  # adjoint: dJ/dx_t
    g = np.zeros_like(u)
    for t in range(N - 2, -1, -1):
        g[t] = 2 * r * u[t] + B.T @ lam
        lam = 2 * np.asarray(Qs[t], float) @ (x[t] - M[t]) + A.T @ lam
    return g


def random_problem(rng, n, m, N, Qs_count=None):
    """A well-conditioned problem: A near the identity, B full rank, SPD precisions, r = 0.1."""
    A = np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n)
    B = rng.standard_normal((n, m)) / np.sqrt(n)
    Qs = []
    for _ in range(Qs_count or N):
        G = rng.standard_normal((n, n))
        Qs.append(G @ G.T / n + 0.5 * np.eye(n))
    mu = rng.standard_normal(N * n)
    return A, B, np.array(Qs), mu, 0.1


def double_integrator(dim, dt):
    """2nd-order point mass in `dim` dimensions: x = [p, v], u = acceleration."""
    I = np.eye(dim)
    A = np.block([[I, dt * I], [np.zeros((dim, dim)), I]])
    B = np.vstack([0.5 * dt * dt * I, dt * I])
    return A, B
