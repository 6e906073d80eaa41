"""An independent, high-precision reference for ilqr_problem_closed_loop_cov_clr (include/ilqr_hip.h "Analytic: ilqr_problem_closed_loop_cov_clr")
-- test infrastructure.

Plain Python on mpmath at 50 decimal digits, restated from the header's text alone; it shares no code with the library and takes only the link
frames from tests/clearance_reference.py.  The covariance is DATA here: the Sigma the library returns (held to tests/closed_loop_cov.py), taken
exactly.  What it states:

  joint m         on segment s_m, axis a_m = R_{s_m} seg_axis (a rotation keeps its axis), origin r_m = the origin of F_{s_m}; it moves link L iff
                  s_m <= L
  pair (i, j)     clr and n as in "clearance" / "obstacle terms"; grad[m] = n . (a_m x (p_i - r_m)) for the joints that move sphere i's link, 0
                  for the others; a self pair (a, b): n = (p_b - p_a) / |p_b - p_a|, grad[m] = n . (a_m x (p_b - r_m)) for the joints that move
                  b's link and not a's, 0 for the others; a zero gradient where the centres coincide
  var, z          var = grad' Sigma[q,q] grad; z = (clr - margin) / sqrt(var) where var > 0, else +inf (clr >= margin) or -inf
  S_abs           sum_ij |grad_i Sigma_ij grad_j|: the scale of the form's rounding
  step, plan      the minimum in z, ties to the lowest (i, j); bad steps first (the lowest k), then (z, k, i, j)

Every gradient it uses is checked against the central difference of its own clearance at h = 1e-20 (`fd_every`: at every n-th state; the
analytic and the differenced gradient agree to 1e-14, see FD_TOL).  It returns, per entry, the bounds the tests hold the library to:
  var_bound = 1e-12 S_abs,    z_bound = 1e-12 / sigma + |z| (0.5e-12 S_abs / var + 4 * 2^-53)
and asserts (unless told that ties are meant) that every centre distance and every | clr - margin | is at least 1e-9, and that every runner-up
gap of a minimum in z and the distance of clr_z_min from z_tol is at least 1000 times the entry's bound: a badly chosen seed fails here, on the
CPU, and never as a disagreement about which of two near-equal pairs is the minimum."""
from __future__ import annotations

import mpmath as mp
import numpy as np

from tests import clearance_reference as cref

mp.mp.dps = 50
MIN_GAP = mp.mpf("1e-9")
FD_H = mp.mpf("1e-20")
# The header's column a_m x (p_i - r_m) is the derivative of Rodrigues' formula for a UNIT axis.  The axes are the descriptor's doubles, unit to a
# few 2^-53 only (the general chains' are irrational), so the derivative of the reference's own FK departs from the definition by that much times
# a lever arm of about a metre: 1e-14 covers it, and any wrong joint, sign or lever is orders of magnitude beyond.  (The differencing itself is
# good to 1e-24: the 50-digit clearance carries some 1e-44 after the chain's products, over 2 h.)
FD_TOL = mp.mpf("1e-14")
REL = mp.mpf("1e-12")
EPS4 = 4 * mp.mpf(2) ** -53


def _v(a):
    return mp.matrix([mp.mpf(float(x)) for x in a])


def _cross(a, b):
    return mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _norm(a):
    return mp.sqrt(_dot(a, a))


def _frames(chain, q, last):
    """link_frames on joint positions that may be mpf (the central difference moves them by 1e-20): the same products, restated."""
    R, p = mp.eye(3), mp.matrix(3, 1)
    out = [(R.copy(), p.copy())]
    for s in range(last + 1):
        p = p + R * _v(chain["seg_xyz"][s])
        R = R * cref._m(np.asarray(chain["seg_R"][s], float).reshape(3, 3))
        j = int(chain["seg_joint"][s])
        if j >= 0:
            K = cref._skew([mp.mpf(float(v)) for v in chain["seg_axis"][s]])
            R = R * (mp.eye(3) + mp.sin(q[j]) * K + (1 - mp.cos(q[j])) * (K * K))
        out.append((R.copy(), p.copy()))
    return out


def pair_clearances(chain, q, spheres, planes, obs, self_pairs, with_grad=True):
    """[(i, j, clr, grad[dof] or None, centre distance or None)] of one state in the order (i, j); q: dof values (float or mpf), all finite."""
    dof = int(chain["dof"])
    last = max(int(l) for l, _, _ in spheres)
    q = [mp.mpf(v) if isinstance(v, mp.mpf) else mp.mpf(float(v)) for v in q]
    fr = _frames(chain, q, last)
    joints = []   # (m, s_m, a_m, r_m)
    for s in range(last + 1):
        m = int(chain["seg_joint"][s])
        if m >= 0:
            R, p = fr[s + 1]
            joints.append((m, s, R * _v(chain["seg_axis"][s]), p))
    n_obs = len(obs)
    centre = [fr[int(l) + 1][1] + fr[int(l) + 1][0] * _v(c) for l, c, _ in spheres]

    def grad(n, w, lo, hi):   # the joints with lo < s_m <= hi
        g = [mp.mpf(0)] * dof
        for m, s, a, r in joints:
            if lo < s <= hi:
                g[m] = _dot(n, _cross(a, w - r))
        return g

    out = []
    for i, (link, _, r) in enumerate(spheres):
        w, r, link = centre[i], mp.mpf(float(r)), int(link)
        for j in range(n_obs):
            if float(obs[j][3]) < 0:
                continue
            d = w - _v(obs[j][:3])
            dist = _norm(d)
            n = d / dist if dist > 0 else mp.matrix(3, 1)
            out.append((i, j, dist - r - mp.mpf(float(obs[j][3])), grad(n, w, -1, link) if with_grad else None, dist))
        for l, (nn, dd) in enumerate(planes):
            n = _v(nn)
            out.append((i, n_obs + l, _dot(n, w) - mp.mpf(float(dd)) - r, grad(n, w, -1, link) if with_grad else None, None))
        for a, b in sorted(self_pairs):
            if b != i:
                continue
            d = w - centre[a]
            dist = _norm(d)
            n = d / dist if dist > 0 else mp.matrix(3, 1)
            out.append((i, n_obs + len(planes) + a, dist - r - mp.mpf(float(spheres[a][2])), grad(n, w, int(spheres[a][0]), link) if with_grad else None, dist))
    return out


def check_gradients(chain, q, spheres, planes, obs, self_pairs, pairs=None):
    """The analytic gradients of a state against the central difference of the reference's own clearances at h = 1e-20."""
    dof = int(chain["dof"])
    pairs = pair_clearances(chain, q, spheres, planes, obs, self_pairs) if pairs is None else pairs
    for m in range(dof):
        qp = [mp.mpf(float(v)) for v in q]
        qm = list(qp)
        qp[m] += FD_H
        qm[m] -= FD_H
        up = pair_clearances(chain, qp, spheres, planes, obs, self_pairs, with_grad=False)
        dn = pair_clearances(chain, qm, spheres, planes, obs, self_pairs, with_grad=False)
        for (i, j, _, g, dist), u, d in zip(pairs, up, dn):
            if dist is not None and dist == 0:
                continue   # coincident centres: the gradient is 0 by definition, not by differentiation
            fd = (u[2] - d[2]) / (2 * FD_H)
            assert abs(fd - g[m]) <= FD_TOL, f"cov clearance reference: pair ({i}, {j}), joint {m}: gradient {mp.nstr(g[m], 20)} against the central difference {mp.nstr(fd, 20)}"


def _moving(chain, spheres):
    last = max(int(l) for l, _, _ in spheres)
    return [int(j) for j in chain["seg_joint"][: last + 1] if int(j) >= 0]


def state(chain, q, Sig, spheres, planes, obs, self_pairs, margin, fd=False, ties=False):
    """The pairs of one step with var, S_abs, z and the bounds: a list of dicts in the order (i, j); None for a bad step."""
    dof = int(chain["dof"])
    if any(not np.isfinite(q[j]) for j in _moving(chain, spheres)) or not np.all(np.isfinite(np.asarray(Sig)[:dof, :dof])):
        return None
    qq = [q[j] if np.isfinite(q[j]) else 0.0 for j in range(dof)]   # joints behind the last sphere's link are not read
    pairs = pair_clearances(chain, qq, spheres, planes, obs, self_pairs)
    if fd:
        check_gradients(chain, qq, spheres, planes, obs, self_pairs, pairs)
    S = [[mp.mpf(float(Sig[i][j])) for j in range(dof)] for i in range(dof)]
    mg = mp.mpf(float(margin))
    out = []
    for i, j, c, g, dist in pairs:
        if not ties:
            assert dist is None or dist >= MIN_GAP, f"cov clearance reference: pair ({i}, {j}): centres {mp.nstr(dist, 5)} apart (< 1e-9): choose another seed"
            assert abs(c - mg) >= MIN_GAP, f"cov clearance reference: pair ({i}, {j}): clearance {mp.nstr(abs(c - mg), 5)} from the margin (< 1e-9): choose another seed"
        terms = [g[a] * S[a][b] * g[b] for a in range(dof) for b in range(dof)]
        var = max(sum(terms), mp.mpf(0))
        s_abs = sum(abs(t) for t in terms)
        if var > 0:
            z = (c - mg) / mp.sqrt(var)
            zb = REL / mp.sqrt(var) + abs(z) * (REL / 2 * s_abs / var + EPS4)
        else:
            z, zb = (mp.inf if c >= mg else -mp.inf), mp.mpf(0)
        out.append(dict(i=i, j=j, clr=c, grad=g, var=var, S_abs=s_abs, z=z, z_bound=zb, var_bound=REL * s_abs))
    return out


def _min(items, key):
    """(the first minimum in z, the gap in z to the first item with a larger z or None)."""
    best = None
    for it in items:
        if best is None or it["z"] < best["z"]:
            best = it
    rivals = [it["z"] for it in items if it is not best and key(it) != key(best)]
    rivals = [z for z in rivals if not (z == best["z"] and abs(z) == mp.inf)]   # infinities that tie are identities (var == 0), not near-ties
    return best, (min(rivals) - best["z"] if rivals else None)


def cov_clearance(chain, Q, Sigma, spheres, planes, obs, self_pairs, traj_per_set, margin, z_tol, fd_every=1, ties=False):
    """The outputs of the call on the plan's joint positions Q[B][T][dof] and the library's Sigma[B][T][n_x][n_x], as a dict of NumPy arrays
    (clr_var, clr_z, clr_z_min, clr_z_at, eligible) with the bounds var_bound, z_bound [B][T] and z_min_bound [B], and `worst_gap`: the smallest
    ratio of a runner-up gap (or of | clr_z_min - z_tol |) to 1000 times its entry's bound."""
    Q, Sigma = np.asarray(Q, float), np.asarray(Sigma, float)
    B, T = Q.shape[0], Q.shape[1]
    obs = np.zeros((B // traj_per_set, 0, 4)) if obs is None else np.asarray(obs, float)
    zt = mp.mpf(float(z_tol))
    var, z = np.empty((B, T)), np.empty((B, T))
    vb, zb = np.zeros((B, T)), np.zeros((B, T))
    zmin, zmb, at, elig = np.empty(B), np.zeros(B), np.empty((B, 3), np.int32), np.zeros(B, np.int32)
    worst = mp.inf

    def gap_ok(gap, bound, what):
        nonlocal worst
        if gap is None or ties or gap == mp.inf:
            return
        if bound > 0:
            worst = min(worst, gap / (1000 * bound))
        assert gap >= 1000 * bound, f"cov clearance reference: {what}: the runner-up lies {mp.nstr(gap, 5)} away (< 1000 bounds of {mp.nstr(bound, 5)}): choose another seed"

    for b in range(B):
        steps, bad = [], []
        for k in range(T):
            prs = state(chain, Q[b, k], Sigma[b, k], spheres, planes, obs[b // traj_per_set], self_pairs, margin, fd=((b * T + k) % fd_every == 0), ties=ties)
            if prs is None:
                var[b, k] = z[b, k] = np.nan
                bad.append(k)
                steps.append(None)
                continue
            if not prs:
                var[b, k], z[b, k] = 0.0, np.inf
                steps.append(dict(z=mp.inf, k=k, i=-1, j=-1, z_bound=mp.mpf(0)))
                continue
            best, gap = _min(prs, lambda it: (it["i"], it["j"]))
            gap_ok(gap, best["z_bound"], f"plan {b}, step {k}")
            var[b, k], z[b, k] = float(best["var"]), float(best["z"])
            vb[b, k], zb[b, k] = float(best["var_bound"]), float(best["z_bound"])
            steps.append(dict(best, k=k) if best["z"] != mp.inf else dict(z=mp.inf, k=k, i=-1, j=-1, z_bound=mp.mpf(0)))
        if bad:
            zmin[b], at[b], elig[b] = np.nan, (bad[0], -1, -1), 0
            continue
        best, gap = _min(steps, lambda it: it["k"])
        if best["z"] == mp.inf:
            zmin[b], at[b], elig[b] = np.inf, (0, -1, -1), int(mp.inf >= zt)
            continue
        gap_ok(gap, best["z_bound"], f"plan {b}")   # (a sphere no joint moves has var == 0 at every step: infinities, which _min does not count)
        if abs(best["z"]) != mp.inf:
            gap_ok(abs(best["z"] - zt), best["z_bound"], f"plan {b}: clr_z_min against z_tol")
        zmin[b], zmb[b], at[b], elig[b] = float(best["z"]), float(best["z_bound"]), (best["k"], best["i"], best["j"]), int(best["z"] >= zt)
    return dict(clr_var=var, clr_z=z, clr_z_min=zmin, clr_z_at=at, eligible=elig, var_bound=vb, z_bound=zb, z_min_bound=zmb, worst_gap=worst)


# ------------------------------------------------------------------------------------------------ the meaning check

def chi2_interval(dof, p):
    """(lo, hi): the two-sided interval of probability 1 - p of a chi-square variable with `dof` degrees of freedom, divided by dof."""
    half = mp.mpf(dof) / 2
    cdf = lambda x: mp.gammainc(half, 0, x / 2, regularized=True)   # noqa: E731
    sd = mp.sqrt(2 * mp.mpf(dof))
    lo = mp.findroot(lambda x: cdf(x) - mp.mpf(p) / 2, dof - 5 * sd)
    hi = mp.findroot(lambda x: (1 - cdf(x)) - mp.mpf(p) / 2, dof + 5 * sd)
    return lo / dof, hi / dof


def curvature_share(chain, q, Sig, sphere, plane, h=mp.mpf("1e-12")):
    """For one sphere against one plane: Var of the second-order term of the clearance under N(0, Sigma[q,q]), tr((H Sigma)^2) / 2, over the
    first-order variance grad' Sigma grad.  H by central second differences of the reference's own clearance."""
    dof = int(chain["dof"])
    q0 = [mp.mpf(float(v)) for v in q[:dof]]
    f = lambda qq: pair_clearances(chain, qq, [sphere], [plane], [], [], with_grad=False)[0][2]   # noqa: E731
    g = pair_clearances(chain, q0, [sphere], [plane], [], [])[0][3]
    S = mp.matrix([[mp.mpf(float(Sig[i][j])) for j in range(dof)] for i in range(dof)])
    H = mp.matrix(dof, dof)
    for a in range(dof):
        for b in range(a, dof):
            def at(sa, sb):
                qq = list(q0)
                qq[a] += sa * h
                qq[b] += sb * h
                return f(qq)
            H[a, b] = H[b, a] = (at(1, 1) - at(1, -1) - at(-1, 1) + at(-1, -1)) / (4 * h * h) if a != b else (at(1, 0) - 2 * f(q0) + at(-1, 0)) / (h * h)
    HS = H * S
    var1 = sum(g[a] * S[a, b] * g[b] for a in range(dof) for b in range(dof))
    var2 = sum(HS[a, b] * HS[b, a] for a in range(dof) for b in range(dof)) / 2
    return var2 / var1, var1
