"""Independent references for the obstacle terms of the stage cost (include/ilqr_hip.h "obstacle terms") -- test infrastructure.

(i)  state_terms / terms: c_obs, its l_x and l_xx on mpmath at 50 decimal digits, stated from the header's text alone:
         h_ij = max(0, margin - clr_ij),  c = w sum h^2,  l_x = -w sum h grad,  l_xx = w sum_{h > 0} grad grad',  grad = n' Jp,
         column m of Jp = a_m x (p_i - r_m) for the joints that move the sphere's link, n = (p - o) / |p - o| or the plane's normal.
     The link frames come from tests/clearance_reference.py (itself stated from the header); a joint's axis in the base frame is its link
     frame's rotation applied to seg_axis (the rotation about an axis leaves the axis where it was), its origin that frame's position.  Nothing
     is shared with the library.  `terms` asserts about its own inputs that every pair lies at least MIN_GAP = 1e-9 from the hinge's kink and
     that every |p_i - o_j| >= 1e-6, so the active set is unambiguous; check_gradient holds l_x to half the central difference of c_obs.
(ii) iteration: one iteration of ILQRRecursive.cpp:68-155 in float64 numpy -- the sweep with `reg`, then the line search with `alpha_floor` --
     on oracle.cost / cost_x / cost_xx / step plus the terms of (i) rounded to double; with `al` the fixed-multiplier terms the header lists for
     ilqr_problem_gains_al.  Every line-search decision records the relative gap between the two costs it compared; `solve` asserts each is at
     least 1e-9, so a library that agrees to rounding must take the same step sizes."""
from __future__ import annotations

import mpmath as mp
import numpy as np

from oracle import oracle as orc
from tests.clearance_reference import link_frames

mp.mp.dps = 50
MIN_GAP = mp.mpf("1e-9")
MIN_DIST = mp.mpf("1e-6")
DECISION_GAP = 1e-9


def _v(a):
    return mp.matrix([mp.mpf(float(x)) for x in a])


def _cross(a, b):
    return mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def state_terms(chain, q, spheres, planes, obs, margin, weight, derivs=True):
    """dict(cost, lx [dof], lxx [dof][dof], kink, dist) of one state at 50 digits: kink = the smallest |margin - clr_ij|, dist the smallest
    |p_i - o_j|.  spheres [(link, c, r)], planes [(n, d)], obs [n_obs][4] of the state's set."""
    dof = int(chain["dof"])
    fr = link_frames(chain, [float(v) for v in q[:dof]])
    joints = []   # (segment, axis in the base frame, origin) of joint m
    for s, j in enumerate(chain["seg_joint"]):
        if int(j) >= 0:
            R, p = fr[s + 1]
            joints.append((s, R * _v(chain["seg_axis"][s]), p))
    mg, w = mp.mpf(float(margin)), mp.mpf(float(weight))
    cost, lx, lxx = mp.mpf(0), [mp.mpf(0)] * dof, mp.zeros(dof, dof)
    kink, dist = mp.inf, mp.inf
    for link, c, r in spheres:
        R, p = fr[int(link) + 1]
        pw = p + R * _v(c)
        pairs = []   # (clearance, normal)
        for o in obs:
            if float(o[3]) < 0:
                continue
            e = pw - _v(o[:3])
            ln = mp.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2)
            dist = min(dist, ln)
            pairs.append((ln - mp.mpf(float(r)) - mp.mpf(float(o[3])), e / ln if ln > 0 else mp.matrix(3, 1)))
        for nn, dd in planes:
            n = _v(nn)
            pairs.append((n[0] * pw[0] + n[1] * pw[1] + n[2] * pw[2] - mp.mpf(float(dd)) - mp.mpf(float(r)), n))
        for clr, n in pairs:
            h = mg - clr
            kink = min(kink, abs(h))
            if h <= 0:
                continue
            cost += h * h
            if derivs:
                g = [mp.mpf(0)] * dof
                for m, (s, a, org) in enumerate(joints):
                    if s <= int(link):
                        col = _cross(a, pw - org)
                        g[m] = n[0] * col[0] + n[1] * col[1] + n[2] * col[2]
                for a_ in range(dof):
                    lx[a_] += h * g[a_]
                    for b_ in range(dof):
                        lxx[a_, b_] += g[a_] * g[b_]
    return dict(cost=w * cost, lx=[-w * v for v in lx], lxx=w * lxx, kink=kink, dist=dist)


def terms(chain, Q, spheres, planes, obs, traj_per_set, margin, weight):
    """cost[n][T], lx[n][T][dof], lxx[n][T][dof][dof] as doubles of the 50-digit values for the joint positions Q[n][T][dof], with `kink` and
    `dist` over all of them; asserts both gaps (see the module text)."""
    Q = np.asarray(Q, float)
    n, T, dof = Q.shape
    cost, lx, lxx = np.empty((n, T)), np.empty((n, T, dof)), np.empty((n, T, dof, dof))
    kink, dist = mp.inf, mp.inf
    for t in range(n):
        for k in range(T):
            r = state_terms(chain, Q[t, k], spheres, planes, obs[t // traj_per_set], margin, weight)
            cost[t, k] = float(r["cost"])
            lx[t, k] = [float(v) for v in r["lx"]]
            lxx[t, k] = np.array([[float(r["lxx"][a, b]) for b in range(dof)] for a in range(dof)])
            kink, dist = min(kink, r["kink"]), min(dist, r["dist"])
    assert kink >= MIN_GAP, f"obstacle reference: a pair lies {mp.nstr(kink, 5)} from the hinge's kink (< 1e-9): choose another seed"
    assert dist >= MIN_DIST, f"obstacle reference: a sphere centre lies {mp.nstr(dist, 5)} from an obstacle's centre (< 1e-6): choose another seed"
    return dict(cost=cost, lx=lx, lxx=lxx, kink=kink, dist=dist)


def check_gradient(chain, q, spheres, planes, obs, margin, weight, step="1e-20", rel="1e-15"):
    """l_x of a state against half the central difference of c_obs, both at 50 digits; returns the worst error relative to max(1, |l_x|)."""
    r = state_terms(chain, q, spheres, planes, obs, margin, weight)
    e = mp.mpf(step)
    worst = mp.mpf(0)
    dof = int(chain["dof"])
    for m in range(dof):
        def c(sign):   # q is taken exactly and moved at 50 digits
            qq = [mp.mpf(float(v)) for v in q[:dof]]
            qq[m] = qq[m] + sign * e
            return _state_cost_mp(chain, qq, spheres, planes, obs, margin, weight)
        half = (c(1) - c(-1)) / (2 * e) / 2
        worst = max(worst, abs(half - r["lx"][m]) / max(1, abs(r["lx"][m])))
    assert worst <= mp.mpf(rel), f"obstacle reference: l_x is {mp.nstr(worst, 5)} from half the central difference of c_obs"
    return worst


def _state_cost_mp(chain, qq, spheres, planes, obs, margin, weight):
    """c_obs at joint positions given as mpf (link_frames takes floats): the frames restated once more, for check_gradient alone."""
    R, p = mp.eye(3), mp.matrix(3, 1)
    frames = [(R.copy(), p.copy())]
    for s in range(len(chain["seg_joint"])):
        p = p + R * _v(chain["seg_xyz"][s])
        R = R * mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(chain["seg_R"][s], float).reshape(3, 3)])
        j = int(chain["seg_joint"][s])
        if j >= 0:
            a = _v(chain["seg_axis"][s])
            K = mp.matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            R = R * (mp.eye(3) + mp.sin(qq[j]) * K + (1 - mp.cos(qq[j])) * (K * K))
        frames.append((R.copy(), p.copy()))
    mg, total = mp.mpf(float(margin)), mp.mpf(0)
    for link, c, r in spheres:
        R, p = frames[int(link) + 1]
        pw = p + R * _v(c)
        for o in obs:
            if float(o[3]) >= 0:
                e = pw - _v(o[:3])
                h = mg - (mp.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2) - mp.mpf(float(r)) - mp.mpf(float(o[3])))
                total += h * h if h > 0 else 0
        for nn, dd in planes:
            n = _v(nn)
            h = mg - (n[0] * pw[0] + n[1] * pw[1] + n[2] * pw[2] - mp.mpf(float(dd)) - mp.mpf(float(r)))
            total += h * h if h > 0 else 0
    return mp.mpf(float(weight)) * total


# ------------------------------------------------------------------------------------------------ (ii) one iteration in float64

class World:
    """The obstacle terms of one instance for `iteration`: chain, spheres, planes, the instance's obstacle set, margin, weight (None: no terms)."""

    def __init__(self, chain, spheres, planes, obs, margin, weight):
        self.chain, self.spheres, self.planes, self.obs, self.margin, self.weight = chain, spheres, planes, obs, margin, weight
        self.dof = int(chain["dof"])

    def at(self, x, derivs=True):
        r = state_terms(self.chain, x[: self.dof], self.spheres, self.planes, self.obs, self.margin, self.weight, derivs)
        assert r["kink"] >= MIN_GAP, f"obstacle reference: a state of the restated solve lies {mp.nstr(r['kink'], 5)} from the hinge's kink"
        d = self.dof
        return float(r["cost"]), np.array([float(v) for v in r["lx"]]), np.array([[float(r["lxx"][a, b]) for b in range(d)] for a in range(d)])


def _stage(s, world, x, u, k):
    c = orc.cost(s, x, u, k)
    return c + world.at(x, derivs=False)[0] if world is not None else c


def rollout(s, world, x0, U):
    """X and the cost of the controls U [T-1][n_u] from x0: ILQRRecursive.cpp:27-56 with c_obs in every stage."""
    T = s.T
    X, cost = [np.asarray(x0, float)], 0.0
    for k in range(T - 1):
        cost += _stage(s, world, X[k], U[k], k)
        X.append(orc.step(s, X[k], U[k])[0])
    cost += _stage(s, world, X[T - 1], np.zeros(s.n_u), T - 1)
    return np.array(X), cost


def iteration(s, R_diag, world, X, U, cost0, reg=1e-6, alpha_floor=1e-3, line_search=True, al=None):
    """One iteration about (X, U) with cost0.  al: dict(A [m][n_x+n_u], b [m], lam [T-1][m], penalty) -- the multipliers stay fixed.  Returns
    dict(X, U, K [T-1][n_u][n_x], d [T-1][n_u] scaled by the accepted alpha, cost, alpha, gaps: the relative gap of every decision)."""
    T, nx, nu = s.T, s.n_x, s.n_u
    R = np.diag(np.asarray(R_diag, float)[:nu])

    def derivs(x, k):
        lx, lxx = orc.cost_x(s, x, k), orc.cost_xx(s, x, k)
        if world is not None:
            _, ox, oxx = world.at(x)
            lx[: world.dof] += ox
            lxx[: world.dof, : world.dof] += oxx
        return lx, lxx

    p, P = derivs(X[T - 1], T - 1)
    K, d = np.zeros((T - 1, nu, nx)), np.zeros((T - 1, nu))
    for k in range(T - 2, -1, -1):
        _, _, A, B, _ = orc.step(s, X[k], U[k])
        lx, lxx = derivs(X[k], k)
        Qux, Quu, Qxx, Qxu = B.T @ P @ A, R + B.T @ P @ B, lxx + A.T @ P @ A, A.T @ P @ B
        Qu, Qx = R @ U[k] + B.T @ p, lx + A.T @ p
        if al is not None:
            for r in range(al["A"].shape[0]):
                cx, cu = al["A"][r, :nx], al["A"][r, nx:]
                g = cx @ X[k] + cu @ U[k] - al["b"][r]
                lam = al["lam"][k, r]
                Ik = al["penalty"] * (0.0 if (g < 0 and lam == 0) else 1.0)
                Quu, Qux, Qxx, Qxu = Quu + Ik * np.outer(cu, cu), Qux + Ik * np.outer(cu, cx), Qxx + Ik * np.outer(cx, cx), Qxu + Ik * np.outer(cx, cu)
                Qu, Qx = Qu + cu * (lam + Ik * g), Qx + cx * (lam + Ik * g)
        Qi = -np.linalg.inv(Quu + reg * np.eye(nu))
        K[k], d[k] = Qi @ Qux, Qi @ Qu
        P = Qxx + K[k].T @ Quu @ K[k] + K[k].T @ Qux + Qxu @ K[k]
        p = Qx + K[k].T @ Quu @ d[k] + K[k].T @ Qu + Qxu @ d[k]
    alpha, gaps = 2.0, []
    while True:
        alpha /= 2.0
        Xn, Un, cost = [X[0].copy()], [], 0.0
        for k in range(T - 1):
            u = U[k] + K[k] @ (Xn[k] - X[k]) + alpha * d[k]
            Un.append(u)
            cost += _stage(s, world, Xn[k], u, k)
            Xn.append(orc.step(s, Xn[k], u)[0])
        cost += _stage(s, world, Xn[T - 1], np.zeros(nu), T - 1)
        if line_search:
            gaps.append(abs(cost - cost0) / max(abs(cost0), 1e-300))
        if not ((cost >= cost0 or np.isnan(cost)) and alpha > alpha_floor and line_search):
            break
    return dict(X=np.array(Xn), U=np.array(Un), K=K, d=alpha * d, cost=cost, alpha=alpha, gaps=gaps)


def solve(s, R_diag, world, x0, U0, nb_iter, reg=1e-6, alpha_floor=1e-3, al=None):
    """nb_iter iterations from U0 (no early stop); asserts the decision gaps.  Returns the last iteration's dict with `alphas` of all of them."""
    U = np.asarray(U0, float).reshape(s.T - 1, s.n_u)
    X, cost = rollout(s, world, x0, U)
    out, alphas = dict(X=X, U=U, cost=cost, alpha=1.0, K=None, d=None), []
    for it in range(nb_iter):
        out = iteration(s, R_diag, world, out["X"], out["U"], out["cost"], reg, alpha_floor, True, al)
        assert all(g >= DECISION_GAP for g in out["gaps"]), f"obstacle reference: iteration {it}: a line-search decision rests on a relative gap of {min(out['gaps']):.3e} (< 1e-9): choose other inputs"
        alphas.append(out["alpha"])
    out["alphas"] = alphas
    return out
