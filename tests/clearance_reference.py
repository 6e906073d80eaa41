"""An independent, high-precision reference for the clearance calls (include/ilqr_hip.h "clearance") -- test infrastructure.

Plain Python on mpmath at 50 decimal digits, as tests/kinematics_reference.py is for the tool pose; it shares no code with the library.  What it
states, it states from the definitions of the header:

  link s          F_s = F_{s-1} Trans(seg_xyz[s]) seg_R[s] Rot(seg_axis[s], q[seg_joint[s]]), F_{-1} = I; no rotation for a fixed segment
  Rot(a, q)       Rodrigues: I + sin(q) [a]x + (1 - cos(q)) [a]x^2, formed from the skew matrix, never from a closed-form 3 x 3 expression
  sphere i        p_i = F_{sph_link[i]} applied to sph_c[i]
  clearance       min over (i, j) of (|p_i - o_j| - r_i) - R_j for the obstacles with R_j >= 0 of the trajectory's set, and of
                  (n_l . p_i - d_l) - r_i for plane l at j = n_obs + l; ties to the lowest i, then the lowest j; +inf without any pair
  trajectory      bad steps first (the lowest k), then (clearance, k, i, j) lexicographic

The inputs are the doubles the library is given (the descriptor's segments, the states, the spheres, planes and obstacles), taken exactly.  Every
minimum comes with the gap to its runner-up, and `clearance` itself asserts (unless told that ties are meant) that every such gap and every
distance of a step's clearance from `margin` is at least MIN_GAP at 50 digits: a badly chosen seed fails here, on the CPU, and never as a
disagreement about which of two near-equal pairs is the minimum."""
from __future__ import annotations

import mpmath as mp
import numpy as np

mp.mp.dps = 50
MIN_GAP = mp.mpf("1e-9")


def _m(a):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a])


def _skew(a):
    return mp.matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def link_frames(chain, q, upto=None):
    """[(R, p)] of the links -1 .. n_seg-1 (index link + 1) at the joint positions q; upto: the last link wanted."""
    R, p = mp.eye(3), mp.matrix(3, 1)
    out = [(R.copy(), p.copy())]
    for s in range(len(chain["seg_joint"]) if upto is None else upto + 1):
        p = p + R * mp.matrix([mp.mpf(float(v)) for v in chain["seg_xyz"][s]])
        R = R * _m(np.asarray(chain["seg_R"][s], float).reshape(3, 3))
        j = int(chain["seg_joint"][s])
        if j >= 0:
            K = _skew([mp.mpf(float(v)) for v in chain["seg_axis"][s]])
            a = mp.mpf(float(q[j]))
            R = R * (mp.eye(3) + mp.sin(a) * K + (1 - mp.cos(a)) * (K * K))
        out.append((R.copy(), p.copy()))
    return out


def state_clearance(chain, q, spheres, planes, obs):
    """(clearance, i, j, gap) of one state: spheres [(link, c, r)], planes [(n, d)], obs [n_obs][4] of the state's set.  (None, -1, -1, None) for a
    bad step (a non-finite position of a joint at or before the last sphere's link); (+inf, -1, -1, None) without any pair."""
    last = max(int(l) for l, _, _ in spheres)
    moving = [int(j) for j in chain["seg_joint"][: last + 1] if int(j) >= 0]
    if any(not np.isfinite(q[j]) for j in moving):
        return None, -1, -1, None
    qq = [q[j] if np.isfinite(q[j]) else 0.0 for j in range(len(q))]   # joints behind the last sphere's link are not read
    fr = link_frames(chain, qq, last)
    n_obs = len(obs)
    pairs = []
    for i, (link, c, r) in enumerate(spheres):
        R, p = fr[int(link) + 1]
        w = p + R * mp.matrix([mp.mpf(float(v)) for v in c])
        r = mp.mpf(float(r))
        for j in range(n_obs):
            if float(obs[j][3]) < 0:
                continue
            o = mp.matrix([mp.mpf(float(v)) for v in obs[j][:3]])
            d = w - o
            pairs.append((mp.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2) - r - mp.mpf(float(obs[j][3])), i, j))
        for l, (nn, dd) in enumerate(planes):
            pairs.append((sum(mp.mpf(float(nn[a])) * w[a] for a in range(3)) - mp.mpf(float(dd)) - r, i, n_obs + l))
    if not pairs:
        return mp.inf, -1, -1, None
    pairs.sort()
    gap = pairs[1][0] - pairs[0][0] if len(pairs) > 1 else None
    return pairs[0][0], pairs[0][1], pairs[0][2], gap


def clearance(chain, Q, spheres, planes, obs, traj_per_set, margin, stats_group=None, ties=False):
    """The outputs of a clearance call on the joint positions Q[n][T][dof] as a dict of NumPy arrays (clr, clr_min, clr_at, n_below, eligible, and
    stats where stats_group is given: the definition's values, its mean summed exactly), with `gap`: the smallest runner-up gap met, over the
    steps' minima and the trajectories' minima, and `margin_gap`: the smallest | clearance - margin | of a good step."""
    Q = np.asarray(Q, float)
    n, T = Q.shape[0], Q.shape[1]
    obs = np.zeros((n // traj_per_set, 0, 4)) if obs is None else np.asarray(obs, float)
    mg = mp.mpf(float(margin))
    clr, cmin, at = np.empty((n, T)), np.empty(n), np.empty((n, 3), np.int32)
    below, elig = np.zeros(n, np.int32), np.zeros(n, np.int32)
    exact_min = []
    gap, margin_gap = mp.inf, mp.inf
    for t in range(n):
        steps = [state_clearance(chain, Q[t, k], spheres, planes, obs[t // traj_per_set]) for k in range(T)]
        bad = [k for k in range(T) if steps[k][0] is None]
        for k, (c, i, j, g) in enumerate(steps):
            clr[t, k] = np.nan if c is None else float(c)
            if c is not None:
                below[t] += int(c < mg)
                if g is not None:
                    gap = min(gap, g)
                if c != mp.inf:
                    margin_gap = min(margin_gap, abs(c - mg))
        if bad:
            cmin[t], at[t], elig[t] = np.nan, (bad[0], -1, -1), 0
            exact_min.append(None)
            continue
        order = sorted((steps[k][0], k) for k in range(T))
        c, k = order[0]
        # A sphere on a link that no joint moves stands still: where it is the minimum, every step repeats the same pair with the same value.  That
        # is an identity, not a near-tie -- the library computes the same bits at every step and the order's rule (the lowest k) decides -- so such
        # steps are no runner-up.
        still = steps[k][1] >= 0 and not any(int(j) >= 0 for j in chain["seg_joint"][: int(spheres[steps[k][1]][0]) + 1])
        rivals = [o[0] for o in order[1:] if not (still and steps[o[1]][1:3] == steps[k][1:3] and o[0] == c)]
        if rivals and c != mp.inf:
            gap = min(gap, rivals[0] - c)
        cmin[t] = float(c)
        at[t] = (0, -1, -1) if c == mp.inf else (k, steps[k][1], steps[k][2])
        elig[t] = int(c >= mg)
        exact_min.append(c)
    if not ties:
        assert gap >= MIN_GAP, f"clearance reference: a minimum's runner-up lies {mp.nstr(gap, 5)} away (< 1e-9): choose another seed"
        assert margin_gap >= MIN_GAP, f"clearance reference: a step's clearance lies {mp.nstr(margin_gap, 5)} from the margin (< 1e-9): choose another seed"
    out = dict(clr=clr, clr_min=cmin, clr_at=at, n_below=below, eligible=elig, gap=gap, margin_gap=margin_gap)
    if stats_group:
        st = np.empty((n // stats_group, 4))
        for g in range(n // stats_group):
            good = [c for c in exact_min[g * stats_group:(g + 1) * stats_group] if c is not None]
            st[g] = (float(sum(good) / len(good)) if good else np.nan, float(min(good)) if good else np.nan, sum(1 for c in good if c < mg),
                     stats_group - len(good))
        out["stats"] = st
    return out
