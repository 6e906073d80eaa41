"""An independent, high-precision forward-kinematics reference for URDF chains -- test infrastructure.

Plain Python on mpmath at DPS decimal digits.  It reads the URDF text itself with xml.etree and shares no code with oracle/oracle.py or
ilqr_planner_amd/csrc/urdf_chain.cpp; what it states, it states from the definitions:

  joint origin        T = Trans(xyz) * Rz(yaw) Ry(pitch) Rx(roll)                      (URDF: rpy are fixed-axis roll, pitch, yaw)
  revolute joint      Rodrigues about the normalised axis: R = I + sin(q) [a]x + (1 - cos(q)) [a]x^2   (URDF default axis 1 0 0)
  tool frame          Trans(tool_xyz) after Rz(tool_rpy[0]) Ry(tool_rpy[1]) Rx(tool_rpy[2])  -- the FIRST entry is the Z angle
  Jacobian            6 x dof, column j = [z_j x (p - o_j); z_j] with z_j, o_j the joint's axis and origin in the base frame
  velocities          [dx; w] = J dq

The rotation products are formed from elementary rotations, never from a closed-form 3 x 3 expression, so that a wrong sign or a transposed
entry in such an expression elsewhere cannot be shared.  The quaternion (w, x, y, z) takes its sign from orocos_kdl's
Rotation::GetQuaternion, restated from its definition: trace > 1e-12 first, then the largest diagonal entry (R00 > R11 and R00 > R22, else
R11 > R22, else R22); the rule is evaluated on the high-precision matrix, and the branch taken and the distance of the nearest comparison
made on the way from its boundary are returned with it.  Eigen's Quaterniond(Matrix3d) rule (trace > 0, else the largest diagonal entry)
is restated the same way for poses seen through an object frame."""
from __future__ import annotations

import xml.etree.ElementTree as ET

import mpmath as mp
import numpy as np

DPS = 50
mp.mp.dps = DPS

KDL_EPS = mp.mpf("1e-12")


def _vec(text, default):
    v = [mp.mpf(t) for t in (text if text is not None else default).split()]
    if len(v) != 3:
        raise ValueError(f"expected three numbers, got {text!r}")
    return v


def Rx(a):
    c, s = mp.cos(a), mp.sin(a)
    return mp.matrix([[1, 0, 0], [0, c, -s], [0, s, c]])


def Ry(a):
    c, s = mp.cos(a), mp.sin(a)
    return mp.matrix([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def Rz(a):
    c, s = mp.cos(a), mp.sin(a)
    return mp.matrix([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def skew(a):
    return mp.matrix([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def rodrigues(axis, q):
    K = skew(axis)
    return mp.eye(3) + mp.sin(q) * K + (1 - mp.cos(q)) * (K * K)


def read_chain(urdf_text, base, tip):
    """The joints on the way from link `base` to link `tip`, base first: dicts(name, moving, xyz, rpy, axis, lower, upper).  axis is
    normalised (None for a fixed joint); a joint without <limit>, or a limit without lower / upper, is unbounded on that side."""
    root = ET.fromstring(urdf_text)
    parent_of = {}
    for j in root.iter("joint"):
        if j.find("child") is not None and j.find("parent") is not None:
            parent_of[j.find("child").get("link")] = j
    joints, link = [], tip
    while link != base:
        if link not in parent_of:
            raise ValueError(f"no chain from {base} to {tip}")
        joints.append(parent_of[link])
        link = parent_of[link].find("parent").get("link")
    out = []
    for j in reversed(joints):
        o, a, lim, typ = j.find("origin"), j.find("axis"), j.find("limit"), j.get("type")
        if typ not in ("revolute", "continuous", "fixed"):
            raise ValueError(f"joint {j.get('name')}: type {typ} is not part of this reference")
        d = dict(name=j.get("name"), moving=typ != "fixed", xyz=_vec(o.get("xyz") if o is not None else None, "0 0 0"),
                 rpy=_vec(o.get("rpy") if o is not None else None, "0 0 0"), axis=None, lower=-mp.inf, upper=mp.inf)
        if d["moving"]:
            ax = _vec(a.get("xyz") if a is not None else None, "1 0 0")
            n = mp.sqrt(sum(c * c for c in ax))
            d["axis"] = [c / n for c in ax]
            if lim is not None and lim.get("lower") is not None:
                d["lower"] = mp.mpf(lim.get("lower"))
            if lim is not None and lim.get("upper") is not None:
                d["upper"] = mp.mpf(lim.get("upper"))
        out.append(d)
    return out


def dof_of(chain):
    return sum(1 for j in chain if j["moving"])


def kdl_quaternion(R):
    """(w, x, y, z) of orocos_kdl's Rotation::GetQuaternion on the matrix R, the branch it took (0: trace, 1 / 2 / 3: R00 / R11 / R22
    largest) and the smallest |difference| of the comparisons it made on the way."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    margin = abs(tr - KDL_EPS)
    if tr > KDL_EPS:
        s = mp.mpf("0.5") / mp.sqrt(tr + 1)
        return [mp.mpf("0.25") / s, (R[2, 1] - R[1, 2]) * s, (R[0, 2] - R[2, 0]) * s, (R[1, 0] - R[0, 1]) * s], 0, margin
    if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        margin = min(margin, abs(R[0, 0] - R[1, 1]), abs(R[0, 0] - R[2, 2]))
        s = 2 * mp.sqrt(1 + R[0, 0] - R[1, 1] - R[2, 2])
        return [(R[2, 1] - R[1, 2]) / s, s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s], 1, margin
    # the first test failed on one (or both) of its comparisons: the nearer of the two that could still flip it
    failed = [abs(R[0, 0] - R[i, i]) for i in (1, 2) if not R[0, 0] > R[i, i]]
    margin = min(margin, min(failed) if len(failed) == 1 else max(failed), abs(R[1, 1] - R[2, 2]))
    if R[1, 1] > R[2, 2]:
        s = 2 * mp.sqrt(1 + R[1, 1] - R[0, 0] - R[2, 2])
        return [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s], 2, margin
    s = 2 * mp.sqrt(1 + R[2, 2] - R[0, 0] - R[1, 1])
    return [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4], 3, margin


def eigen_quaternion(R):
    """(w, x, y, z) of Eigen's Quaterniond(Matrix3d) on R, the branch (0: trace > 0, else 1 + index of the largest diagonal entry) and the
    smallest |difference| of the comparisons made."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    margin = abs(tr)
    if tr > 0:
        t = mp.sqrt(tr + 1)
        return [t / 2, (R[2, 1] - R[1, 2]) / (2 * t), (R[0, 2] - R[2, 0]) / (2 * t), (R[1, 0] - R[0, 1]) / (2 * t)], 0, margin
    i = 0
    margin = min(margin, abs(R[1, 1] - R[0, 0]))
    if R[1, 1] > R[0, 0]:
        i = 1
    margin = min(margin, abs(R[2, 2] - R[i, i]))
    if R[2, 2] > R[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = mp.sqrt(R[i, i] - R[j, j] - R[k, k] + 1)
    c = [None] * 3
    c[i] = t / 2
    c[j] = (R[j, i] + R[i, j]) / (2 * t)
    c[k] = (R[k, i] + R[i, k]) / (2 * t)
    return [(R[k, j] - R[j, k]) / (2 * t)] + c, 1 + i, margin


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def pose(chain, q, tool_rpy=(0, 0, 0), tool_xyz=(0, 0, 0), want_joints=False):
    """Position (3 mpf) and rotation (mp.matrix) of the tool frame at joint angles q; with want_joints also every moving joint's origin
    and axis in the base frame."""
    R, p = mp.eye(3), mp.matrix(3, 1)
    org, axs = [], []
    k = 0
    for j in chain:
        p = p + R * mp.matrix(j["xyz"])
        R = R * (Rz(j["rpy"][2]) * Ry(j["rpy"][1]) * Rx(j["rpy"][0]))
        if j["moving"]:
            org.append([p[i] for i in range(3)])
            z = R * mp.matrix(j["axis"])
            axs.append([z[i] for i in range(3)])
            R = R * rodrigues(j["axis"], mp.mpf(q[k]))
            k += 1
    if k != len(q):
        raise ValueError(f"{len(q)} joint angles for a chain of {k} moving joints")
    p = p + R * mp.matrix([mp.mpf(v) for v in tool_xyz])
    R = R * (Rz(mp.mpf(tool_rpy[0])) * Ry(mp.mpf(tool_rpy[1])) * Rx(mp.mpf(tool_rpy[2])))
    p = [p[i] for i in range(3)]
    return (p, R, org, axs) if want_joints else (p, R)


def jacobian(p, org, axs):
    """6 x dof mp.matrix, column j = [z_j x (p - o_j); z_j]"""
    J = mp.matrix(6, len(org))
    for j, (o, z) in enumerate(zip(org, axs)):
        lin = _cross(z, [p[i] - o[i] for i in range(3)])
        for i in range(3):
            J[i, j], J[3 + i, j] = lin[i], z[i]
    return J


def _np(v):
    return np.array([float(x) for x in v])


def _np2(M):
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])


def fk(chain, q, tool_rpy=(0, 0, 0), tool_xyz=(0, 0, 0), dq=None, frame=None):
    """Everything the tests compare at one configuration, rounded to double at the very end: dict(pos[3], R[3][3], quat[4] (w, x, y, z),
    branch, margin (float), J[6][dof], dx[3], w[3]) and the mpmath values under "mp".  q (and dq) are taken as the exact doubles given.
    frame = (R_f, t_f), a 3 x 3 rotation and an origin: the pose as seen from that object frame, p' = R_f^T (p - t_f), R' = R_f^T R,
    J' = blkdiag(R_f^T, R_f^T) J, with the quaternion's sign by Eigen's rule instead of orocos_kdl's."""
    p, R, org, axs = pose(chain, q, tool_rpy, tool_xyz, want_joints=True)
    J = jacobian(p, org, axs)
    if frame is not None:
        Rf = mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.asarray(frame[0], float)])
        tf = [mp.mpf(float(v)) for v in frame[1]]
        pm = Rf.T * mp.matrix([p[i] - tf[i] for i in range(3)])
        p, R = [pm[i] for i in range(3)], Rf.T * R
        Jn = mp.matrix(6, J.cols)
        for blk in (0, 3):
            Jn[blk:blk + 3, :] = Rf.T * J[blk:blk + 3, :]
        J = Jn
        quat, branch, margin = eigen_quaternion(R)
    else:
        quat, branch, margin = kdl_quaternion(R)
    dqm = mp.matrix([mp.mpf(float(v)) for v in (dq if dq is not None else [0.0] * J.cols)])
    v = J * dqm
    return dict(pos=_np(p), R=_np2(R), quat=_np(quat), branch=branch, margin=float(margin), J=_np2(J), dx=_np([v[i] for i in range(3)]),
                w=_np([v[3 + i] for i in range(3)]), mp=dict(pos=p, R=R, quat=quat, J=J))


BOUNDARY = 1e-9  # a sample whose branch decision lies this close to its boundary may come out with the other sign in double arithmetic


def assert_pose(ref, pos, quat, J=None, atol=1e-12, what=""):
    """pos, quat (and J) of an implementation under test against fk()'s result `ref`, absolute.  The quaternion is compared with its
    sign, except where the reference's branch decision lies within BOUNDARY of its boundary: then up to sign, and True is returned (the
    caller counts these)."""
    assert np.max(np.abs(np.asarray(pos) - ref["pos"])) <= atol, (what, "position", pos, ref["pos"])
    quat = np.asarray(quat)
    near = ref["margin"] <= BOUNDARY
    dq = np.max(np.abs(quat - ref["quat"]))
    if near:
        dq = min(dq, np.max(np.abs(quat + ref["quat"])))
    assert dq <= atol, (what, "quaternion", quat, ref["quat"], "branch", ref["branch"], "margin", ref["margin"])
    if J is not None:
        assert np.asarray(J).shape == ref["J"].shape and np.max(np.abs(np.asarray(J) - ref["J"])) <= atol, (what, "Jacobian", J, ref["J"])
    return bool(near)


def _vee(S):
    return [(S[2, 1] - S[1, 2]) / 2, (S[0, 2] - S[2, 0]) / 2, (S[1, 0] - S[0, 1]) / 2]


def self_check(chain, q, tool_rpy=(0, 0, 0), tool_xyz=(0, 0, 0), h="1e-15"):
    """The reference against itself at one configuration: (largest |entry| of the analytic Jacobian minus central differences of its own
    position and of R'(q) R^T at step h, largest |entry| of R R^T - I)."""
    h = mp.mpf(h)
    q = [mp.mpf(float(v)) for v in q]
    p, R, org, axs = pose(chain, q, tool_rpy, tool_xyz, want_joints=True)
    J = jacobian(p, org, axs)
    worst = mp.mpf(0)
    for j in range(len(q)):
        qp, qm = list(q), list(q)
        qp[j] += h
        qm[j] -= h
        pp, Rp = pose(chain, qp, tool_rpy, tool_xyz)
        pm, Rm = pose(chain, qm, tool_rpy, tool_xyz)
        lin = [(pp[i] - pm[i]) / (2 * h) for i in range(3)]
        ang = _vee(((Rp - Rm) / (2 * h)) * R.T)
        worst = max([worst] + [abs(lin[i] - J[i, j]) for i in range(3)] + [abs(ang[i] - J[3 + i, j]) for i in range(3)])
    E = R * R.T - mp.eye(3)
    return float(worst), float(max(abs(E[i, j]) for i in range(3) for j in range(3)))
