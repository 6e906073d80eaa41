"""Independent references for self-collision pairs in the clearance calls and the obstacle terms (include/ilqr_hip.h "clearance" and "obstacle
terms") -- test infrastructure.

Plain Python on mpmath at 50 decimal digits, stated from the header's text alone; of the other references only link_frames (the link frames of
tests/clearance_reference.py) and the float64 `iteration` / `solve` of tests/obstacle_reference.py are used, the latter with the World of this
file, whose `at` adds the self terms.  Nothing is shared with the library.

  pair (a, b)     clr_ab = (|p_b - p_a| - r_b) - r_a; in a state's minimum it is the pair (i, j) = (b, n_obs + n_planes + a), so a plain sort of
                  (clearance, i, j) gives ties to the lowest i, then the lowest j
  term            h_ab = max(0, margin - clr_ab), c += w h^2, l_x -= w h grad, l_xx += w grad grad' (h > 0),
                  grad[m] = n_ab . (a_m x (p_b - r_m)) for the joints m on a segment s with sph_link[a] < s <= sph_link[b], 0 for every other joint

What the references assert about their own inputs: every pair at least MIN_GAP = 1e-9 from the hinge's kink, every centre distance at least
MIN_DIST = 1e-6, every minimum's runner-up at least MIN_GAP away (unless ties are meant), and -- in obstacle_reference.solve -- every line-search
decision on a relative gap of at least 1e-9.  check_gradient holds l_x to half the central difference of the cost at 50 digits."""
from __future__ import annotations

import mpmath as mp
import numpy as np

from tests.clearance_reference import link_frames

mp.mp.dps = 50
MIN_GAP = mp.mpf("1e-9")
MIN_DIST = mp.mpf("1e-6")


def _v(a):
    return mp.matrix([mp.mpf(float(x)) for x in a])


def _cross(a, b):
    return mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _norm(e):
    return mp.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2)


def _centres(fr, spheres):
    return [fr[int(link) + 1][1] + fr[int(link) + 1][0] * _v(c) for link, c, _ in spheres]


def _pairs(centres, spheres, planes, obs, self_pairs):
    """[(clearance, i, j, normal, kind)] of a state in no particular order; kind 'o', 'p' or the anchor a of a self pair."""
    n_obs = len(obs)
    out = []
    for i, (link, c, r) in enumerate(spheres):
        w, r = centres[i], mp.mpf(float(r))
        for j in range(n_obs):
            if float(obs[j][3]) < 0:
                continue
            e = w - _v(obs[j][:3])
            ln = _norm(e)
            out.append((ln - r - mp.mpf(float(obs[j][3])), i, j, e / ln if ln > 0 else mp.matrix(3, 1), "o", ln))
        for l, (nn, dd) in enumerate(planes):
            n = _v(nn)
            out.append((n[0] * w[0] + n[1] * w[1] + n[2] * w[2] - mp.mpf(float(dd)) - r, i, n_obs + l, n, "p", None))
    for a, b in self_pairs:
        e = centres[b] - centres[a]
        ln = _norm(e)
        out.append((ln - mp.mpf(float(spheres[b][2])) - mp.mpf(float(spheres[a][2])), int(b), n_obs + len(planes) + int(a),
                    e / ln if ln > 0 else mp.matrix(3, 1), int(a), ln))
    return out


# ------------------------------------------------------------------------------------------------ clearance

def state_clearance(chain, q, spheres, planes, obs, self_pairs):
    """(clearance, i, j, gap) of one state; (None, -1, -1, None) for a bad step; (+inf, -1, -1, None) without any pair."""
    last = max(int(l) for l, _, _ in spheres)
    moving = [int(j) for j in chain["seg_joint"][: last + 1] if int(j) >= 0]
    if any(not np.isfinite(q[j]) for j in moving):
        return None, -1, -1, None
    qq = [q[j] if np.isfinite(q[j]) else 0.0 for j in range(len(q))]   # joints behind the last sphere's link are not read
    fr = link_frames(chain, qq, last)
    pairs = sorted((p[0], p[1], p[2]) for p in _pairs(_centres(fr, spheres), spheres, planes, obs, self_pairs))
    if not pairs:
        return mp.inf, -1, -1, None
    return pairs[0][0], pairs[0][1], pairs[0][2], (pairs[1][0] - pairs[0][0] if len(pairs) > 1 else None)


def clearance(chain, Q, spheres, planes, obs, self_pairs, traj_per_set, margin, ties=False):
    """The outputs of a clearance call on the joint positions Q[n][T][dof]: clr, clr_min, clr_at, n_below, eligible, with `gap` (the smallest
    runner-up gap over the steps' and the trajectories' minima), `margin_gap` and `step_at` [n][T][2]: the pair (i, j) of every step's minimum.  Trajectories: bad steps first (the lowest k), then
    (clearance, k, i, j) lexicographic."""
    Q = np.asarray(Q, float)
    n, T = Q.shape[0], Q.shape[1]
    obs = np.zeros((n // traj_per_set, 0, 4)) if obs is None else np.asarray(obs, float)
    mg = mp.mpf(float(margin))
    clr, cmin, at = np.empty((n, T)), np.empty(n), np.empty((n, 3), np.int32)
    below, elig = np.zeros(n, np.int32), np.zeros(n, np.int32)
    step_at = np.empty((n, T, 2), np.int32)
    gap, margin_gap = mp.inf, mp.inf
    for t in range(n):
        steps = [state_clearance(chain, Q[t, k], spheres, planes, obs[t // traj_per_set], self_pairs) for k in range(T)]
        bad = [k for k in range(T) if steps[k][0] is None]
        for k, (c, i, j, g) in enumerate(steps):
            clr[t, k] = np.nan if c is None else float(c)
            step_at[t, k] = (i, j)
            if c is not None:
                below[t] += int(c < mg)
                if g is not None:
                    gap = min(gap, g)
                if c != mp.inf:
                    margin_gap = min(margin_gap, abs(c - mg))
        if bad:
            cmin[t], at[t], elig[t] = np.nan, (bad[0], -1, -1), 0
            continue
        order = sorted((steps[k][0], k) for k in range(T))
        c, k = order[0]
        # A sphere that no joint moves repeats the same pair with the same value at every step (an obstacle or a plane: the second member of a
        # self pair always moves): an identity that the order's rule (the lowest k) decides, not a near-tie.
        still = steps[k][1] >= 0 and not any(int(j) >= 0 for j in chain["seg_joint"][: int(spheres[steps[k][1]][0]) + 1])
        rivals = [o[0] for o in order[1:] if not (still and steps[o[1]][1:3] == steps[k][1:3] and o[0] == c)]
        if rivals and c != mp.inf:
            gap = min(gap, rivals[0] - c)
        cmin[t] = float(c)
        at[t] = (0, -1, -1) if c == mp.inf else (k, steps[k][1], steps[k][2])
        elig[t] = int(c >= mg)
    if not ties:
        assert gap >= MIN_GAP, f"self-collision reference: a minimum's runner-up lies {mp.nstr(gap, 5)} away (< 1e-9): choose another seed"
        assert margin_gap >= MIN_GAP, f"self-collision reference: a step's clearance lies {mp.nstr(margin_gap, 5)} from the margin (< 1e-9): choose another seed"
    return dict(clr=clr, clr_min=cmin, clr_at=at, n_below=below, eligible=elig, gap=gap, margin_gap=margin_gap, step_at=step_at)


# ------------------------------------------------------------------------------------------------ terms

def _frames_mp(chain, qq):
    """The link frames at joint positions given as mpf (link_frames takes floats): restated once more, for check_gradient alone."""
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
    return frames


def _cost_of_frames(fr, spheres, planes, obs, self_pairs, margin, weight):
    mg, total = mp.mpf(float(margin)), mp.mpf(0)
    for p in _pairs(_centres(fr, spheres), spheres, planes, obs, self_pairs):
        h = mg - p[0]
        total += h * h if h > 0 else 0
    return mp.mpf(float(weight)) * total


def state_terms(chain, q, spheres, planes, obs, self_pairs, margin, weight, derivs=True):
    """dict(cost, lx [dof], lxx [dof][dof], kink, dist, self_active) of one state at 50 digits: kink = the smallest |margin - clr| over all pairs,
    dist the smallest centre distance of an obstacle or self pair, self_active the number of self pairs with h > 0."""
    dof = int(chain["dof"])
    fr = link_frames(chain, [float(v) for v in q[:dof]])
    joints = []   # (segment, axis in the base frame, origin) of joint m
    for s, j in enumerate(chain["seg_joint"]):
        if int(j) >= 0:
            R, p = fr[s + 1]
            joints.append((s, R * _v(chain["seg_axis"][s]), p))
    centres = _centres(fr, spheres)
    mg, w = mp.mpf(float(margin)), mp.mpf(float(weight))
    cost, lx, lxx = mp.mpf(0), [mp.mpf(0)] * dof, mp.zeros(dof, dof)
    kink, dist, self_active = mp.inf, mp.inf, 0
    for clr, i, j, n, kind, ln in _pairs(centres, spheres, planes, obs, self_pairs):
        if ln is not None:
            dist = min(dist, ln)
        h = mg - clr
        kink = min(kink, abs(h))
        if h <= 0:
            continue
        cost += h * h
        self_active += isinstance(kind, int)
        if derivs:
            link_i = int(spheres[i][0])
            behind = int(spheres[kind][0]) if isinstance(kind, int) else -1   # a self pair: only the joints behind the anchor's link move b against a
            g = [mp.mpf(0)] * dof
            for m, (s, a, org) in enumerate(joints):
                if behind < s <= link_i:
                    col = _cross(a, centres[i] - org)
                    g[m] = n[0] * col[0] + n[1] * col[1] + n[2] * col[2]
            for a_ in range(dof):
                lx[a_] += h * g[a_]
                for b_ in range(dof):
                    lxx[a_, b_] += g[a_] * g[b_]
    return dict(cost=w * cost, lx=[-w * v for v in lx], lxx=w * lxx, kink=kink, dist=dist, self_active=self_active)


def terms(chain, Q, spheres, planes, obs, self_pairs, traj_per_set, margin, weight):
    """cost[n][T], lx[n][T][dof], lxx[n][T][dof][dof] as doubles of the 50-digit values for Q[n][T][dof], with `kink` and `dist`; asserts both."""
    Q = np.asarray(Q, float)
    n, T, dof = Q.shape
    obs = np.zeros((n // traj_per_set, 0, 4)) if obs is None else np.asarray(obs, float)
    cost, lx, lxx = np.empty((n, T)), np.empty((n, T, dof)), np.empty((n, T, dof, dof))
    kink, dist, self_active = mp.inf, mp.inf, 0
    for t in range(n):
        for k in range(T):
            r = state_terms(chain, Q[t, k], spheres, planes, obs[t // traj_per_set], self_pairs, margin, weight)
            self_active += r["self_active"]
            cost[t, k] = float(r["cost"])
            lx[t, k] = [float(v) for v in r["lx"]]
            lxx[t, k] = np.array([[float(r["lxx"][a, b]) for b in range(dof)] for a in range(dof)])
            kink, dist = min(kink, r["kink"]), min(dist, r["dist"])
    assert kink >= MIN_GAP, f"self-collision reference: a pair lies {mp.nstr(kink, 5)} from the hinge's kink (< 1e-9): choose another seed"
    assert dist >= MIN_DIST, f"self-collision reference: two centres lie {mp.nstr(dist, 5)} apart (< 1e-6): choose another seed"
    return dict(cost=cost, lx=lx, lxx=lxx, kink=kink, dist=dist, self_active=self_active)


def check_gradient(chain, q, spheres, planes, obs, self_pairs, margin, weight, step="1e-20", rel="1e-15"):
    """l_x of a state against half the central difference of the cost, both at 50 digits; returns the worst error relative to max(1, |l_x|)."""
    r = state_terms(chain, q, spheres, planes, obs, self_pairs, margin, weight)
    assert r["cost"] > 0, "self-collision reference: no pair is active at the state of check_gradient"
    e = mp.mpf(step)
    worst = mp.mpf(0)
    dof = int(chain["dof"])
    for m in range(dof):
        def c(sign):   # q is taken exactly and moved at 50 digits
            qq = [mp.mpf(float(v)) for v in q[:dof]]
            qq[m] = qq[m] + sign * e
            return _cost_of_frames(_frames_mp(chain, qq), spheres, planes, obs, self_pairs, margin, weight)
        half = (c(1) - c(-1)) / (2 * e) / 2
        worst = max(worst, abs(half - r["lx"][m]) / max(1, abs(r["lx"][m])))
    assert worst <= mp.mpf(rel), f"self-collision reference: l_x is {mp.nstr(worst, 5)} from half the central difference of the cost"
    return worst


class World:
    """The obstacle and self terms of one instance for obstacle_reference.iteration / solve: what their World is, with `at` adding the self terms."""

    def __init__(self, chain, spheres, planes, obs, self_pairs, margin, weight):
        self.chain, self.spheres, self.planes, self.obs, self.self_pairs, self.margin, self.weight = chain, spheres, planes, obs, self_pairs, margin, weight
        self.dof = int(chain["dof"])

    def at(self, x, derivs=True):
        r = state_terms(self.chain, x[: self.dof], self.spheres, self.planes, self.obs, self.self_pairs, self.margin, self.weight, derivs)
        assert r["kink"] >= MIN_GAP, f"self-collision reference: a state of the restated solve lies {mp.nstr(r['kink'], 5)} from the hinge's kink"
        assert r["dist"] >= MIN_DIST, f"self-collision reference: a state of the restated solve has two centres {mp.nstr(r['dist'], 5)} apart"
        d = self.dof
        return float(r["cost"]), np.array([float(v) for v in r["lx"]]), np.array([[float(r["lxx"][a, b]) for b in range(d)] for a in range(d)])
