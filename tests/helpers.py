"""Shared test helpers: load golden fixtures, build oracle Systems, synthetic batches."""
from __future__ import annotations

import glob
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as orc  # noqa: E402  (tests are allowed to use the oracle)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def hostsim_sources():
    """The host sources of the library, as tests/tools/hostsim/build.sh lists them: the lane-per-instance kernels, every unit of the C-ABI
    orchestration (ilqr_capi*.cpp), the URDF reader and the stubs of everything else."""
    hostsim = os.path.join(ROOT, "tests", "tools", "hostsim")
    src = os.path.join(ROOT, "ilqr_planner_amd", "csrc")
    return ([os.path.join(src, "ilqr_kernels.hip")] + sorted(glob.glob(os.path.join(src, "ilqr_capi*.cpp"))) +
            [os.path.join(src, "urdf_chain.cpp"), os.path.join(hostsim, "stubs.cpp")])


def build_hostsim(lib):
    """The lane-per-instance kernels and the C-ABI orchestration built with g++ into the shared library `lib`: the sources and include paths
    of tests/tools/hostsim/build.sh, without sanitizers.  Returns `lib`."""
    hostsim = os.path.join(ROOT, "tests", "tools", "hostsim")
    src = os.path.join(ROOT, "ilqr_planner_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + hostsim, "-I" + src, "-Wno-unused-result", "-x", "c++",
                           *hostsim_sources(), "-o", str(lib)])
    return str(lib)


def urdf_text():
    return open(os.path.join(GOLDEN, "panda_chain.urdf")).read()


def golden():
    return json.load(open(os.path.join(GOLDEN, "traces.json")))


def panda_segs(tool_rpy=(0, 0, 0), tool_xyz=(0, 0, 0)):
    return orc.chain_from_urdf(urdf_text(), "panda_link0", "panda_tip", tool_rpy, tool_xyz)


# Hand-written chains that are not the Panda (tests/golden/chains/): name -> (file, base link, tip link).  "gen4cut3" is gen4 cut at the
# link behind its third moving joint.
GENERAL_CHAINS = {"gen7": ("gen7.urdf", "g7_base", "g7_tip"), "gen4": ("gen4.urdf", "g4_base", "g4_tip"), "gen4cut3": ("gen4.urdf", "g4_base", "g4_l3")}
TOOL_FRAMES = {"identity": (None, None), "rotated": ([2.8, -0.4, 1.3], [0.02, -0.03, 0.07])}  # tool_rpy (its first entry is the Z angle), tool_xyz


def general_chain_text(name):
    return open(os.path.join(GOLDEN, "chains", GENERAL_CHAINS[name][0])).read()


def chain_pair(urdf_text_, base, tip, tool_rpy=None, tool_xyz=None):
    """(chain, segs) of one URDF chain with one tool frame: the `chain` dict of workloads.make_batch / capi.make_desc from the library's
    own reader, and the oracle's `segs` from the oracle's reader."""
    from ilqr_planner_amd import capi

    zero = (0.0, 0.0, 0.0)
    return (capi.chain_from_urdf(urdf_text_, base, tip, tool_rpy, tool_xyz),
            orc.chain_from_urdf(urdf_text_, base, tip, tool_rpy if tool_rpy is not None else zero, tool_xyz if tool_xyz is not None else zero))


def general_chain(name, tool="identity"):
    """chain_pair of one of GENERAL_CHAINS with one of TOOL_FRAMES"""
    _, base, tip = GENERAL_CHAINS[name]
    return chain_pair(general_chain_text(name), base, tip, *TOOL_FRAMES[tool])


def object_frames():
    """Two object frames (4 x 4 poses) for keypoints seen through a frame: a general rotation, and one 0.15 rad short of a half turn about
    the oblique axis (1, 2, -2) / 3, so that a tool near the base orientation is seen with a negative trace."""
    out = []
    for axis, th, t in (([2.0, -1.0, 3.0], 0.9, [0.3, -0.2, 0.25]), ([1.0, 2.0, -2.0], np.pi - 0.15, [0.1, 0.35, 0.2])):
        a = np.asarray(axis) / np.linalg.norm(axis)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        T = np.eye(4)
        T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        T[:3, 3] = t
        out.append(T)
    return out


def oracle_system(prob, segs=None):
    segs = segs or panda_segs()
    kind = orc.SYS_POS_ORN if prob["kind"] == "POS_ORN" else orc.SYS_POS_ORN_TIME
    kps = []
    for k in prob["keypoints"]:
        d = dict(k)
        d["Q"] = np.diag(k["Qdiag"]) if "Qdiag" in k else np.asarray(k["Q"])
        kps.append(d)
    return orc.make_system(segs, kind, prob["nb_deriv"], prob["T"], prob["dt"], prob["R_diag"], kps, prob["q0"], prob["dq0"],
                           prob.get("qMax"), prob.get("qMin"), prob.get("dqMax"), prob.get("dqMin"), prob.get("lim_mult", 1))


def u0_of(prob):
    return np.tile(np.asarray(prob["u0_step"], float), prob["T"] - 1)


def psi_of(spec, T, n_u):
    """PSI matrices exactly as the tutorial cells build them."""
    K = spec["K"]
    if spec["kind"] in ("unitstep", "sawtooth", "rbf", "bernstein"):
        return np.kron(orc.psi(spec["kind"], T - 1, K), np.eye(n_u))
    if spec["kind"] == "sawtooth+unitstep_dt":
        a = np.diag([1.0] * (n_u - 1) + [0.0])
        b = np.diag([0.0] * (n_u - 1) + [1.0])
        return np.kron(orc.psi("sawtooth", T - 1, K), a) + np.kron(orc.psi("unitstep", T - 1, K), b)
    raise KeyError(spec["kind"])


def sig6(x):
    """Value as the reference prints it (default ostream precision 6)."""
    return float("%.6g" % x)


def assert_trace(got_cost, got_alpha, trace, ulps=0.51):
    assert len(got_cost) == len(trace), (len(got_cost), len(trace))
    for i, ((c_ref, a_ref), c, a) in enumerate(zip(trace, got_cost, got_alpha)):
        assert sig6(a) == a_ref, f"iteration {i+1}: alpha {a} != {a_ref}"
        if c_ref is None:
            assert np.isnan(c), f"iteration {i+1}: expected nan, got {c}"
        else:
            # the printed value has 6 significant digits: allow half a unit in the last place (+ slack for rounding ties)
            ulp6 = 10.0 ** (np.floor(np.log10(abs(c_ref))) - 5)
            assert abs(c - c_ref) <= ulps * ulp6, f"iteration {i+1}: cost {c!r} vs {c_ref!r}"


# ----------------------------------------------------------------------------- synthetic batches (ilqr_planner_amd.workloads) -> oracle


def oracle_system_of_instance(cfg, inp, i, segs=None):
    """Oracle System for instance i of a batch made by ilqr_planner_amd.workloads.make_batch."""
    if cfg["kind"] in (2, 3):  # JointSpace(Time)PlannerSys with its TRUE number of joints (the device batch is padded to 7)
        n = inp.get("dof", 7)
        tm = cfg["kind"] == 3
        segs_j = dict(dof=n, seg_joint=list(range(n)), seg_xyz=[[0, 0, 0]] * n, seg_axis=[[0, 0, 1]] * n, seg_R=[[1, 0, 0, 0, 1, 0, 0, 0, 1]] * n)
        kps = []
        for k, ts in enumerate(inp["kp_t"]):
            qd = list(cfg["Qdiag"][k][:n]) + ([cfg["Qdiag"][k][-1]] if tm else [])
            d = dict(timestep=ts, target=inp["targets"][k][i][:n], Q=np.diag(qd))
            if tm:
                d["ctime"] = inp["targets"][k][i][-1]
            kps.append(d)
        lim = inp["limits"]
        return orc.make_system(segs_j, orc.SYS_JOINT_TIME if tm else orc.SYS_JOINT, 1, cfg["T"], cfg["dt"], [1e-5] * (n + (1 if tm else 0)), kps,
                               inp["q0"][i][:n], [0.0] * n, lim["state_max"][:n], lim["state_min"][:n])
    segs = segs or panda_segs()
    nd = cfg["nb_deriv"]
    tm = cfg["kind"] == 1
    kps = []
    for k, ts in enumerate(inp["kp_t"]):
        tg = inp["targets"][k][i]
        d = dict(timestep=ts, pos=tg[0:3], orn=tg[3:7], Q=np.diag(cfg["Qdiag"][k]))
        if nd == 2:
            d.update(dpos=tg[7:10], dorn=tg[10:14])
        if tm:
            d["ctime"] = tg[-1]
        if cfg.get("kp_dist") and cfg["kp_dist"][k] is not None:
            d["dist"] = cfg["kp_dist"][k]  # PosOrnKeypointDistFunct
        if cfg.get("kp_frames") and cfg["kp_frames"][k] is not None:
            d["frame"] = cfg["kp_frames"][k]  # 4 x 4 pose of the object frame the keypoint's sub-system works in
        if cfg.get("hybrid"):  # workloads "C2h"/"C4h": joint-space via point of a JointSpace(Time)PlannerSys sub-system, then a pose goal
            nu_ = 7 + (1 if tm else 0)
            if k == 0:
                d = dict(timestep=ts, joint=True, target=tg[:7], Q=np.diag(cfg["Qdiag"][k]), Ru=[1e-3] * nu_)
                if tm:
                    d["ctime"] = tg[-1]
            else:
                d["Ru"] = [1e-5] * nu_
        kps.append(d)
    dof = 7
    lim = inp["limits"]
    qMax, qMin = lim["state_max"][:dof], lim["state_min"][:dof]
    dqMax = lim["state_max"][dof:2 * dof] if nd == 2 else None
    dqMin = lim["state_min"][dof:2 * dof] if nd == 2 else None
    nu = dof + (1 if tm else 0)
    from ilqr_planner_amd.workloads import control_weights
    return orc.make_system(segs, orc.SYS_POS_ORN_TIME if tm else orc.SYS_POS_ORN, nd, cfg["T"], cfg["dt"], control_weights(cfg, nu), kps,
                           inp["q0"][i], inp["dq0"][i], qMax, qMin, dqMax, dqMin,
                           lim_mult=(1 if cfg.get("limits2") else 2) if cfg.get("hybrid") else 1,
                           limits2=dict(qMax=np.asarray(qMax) - 0.3, qMin=np.asarray(qMin) + 0.3) if cfg.get("limits2") else None)


def oracle_solve_instance(cfg, inp, i, nb_iter, early_stop, segs=None):
    """The oracle's own run of instance i, with the solver constants of the case (cfg["constants"], absent = the reference's)."""
    consts = cfg.get("constants")
    s = oracle_system_of_instance(cfg, inp, i, segs)
    U0 = inp["U0"][i]
    if cfg["kind"] in (2, 3) and inp.get("dof", 7) < 7:  # joint-space batches are padded to 7 joints on the device only
        n = inp["dof"]
        U0 = np.hstack([U0[:, :n], U0[:, 7:]])
    U0 = U0.reshape(-1)
    if cfg["solver"] == "recursive":
        return orc.solve_recursive(s, U0, nb_iter, True, early_stop, constants=consts)
    if cfg["solver"] == "al":
        al = cfg["al"]
        return orc.solve_al(s, inp["A"], inp["b"], inp["lambda0"][i], U0, nb_iter, al["lag"], al["penalty"], al["scaling"], True, early_stop,
                            constants=consts)
    raise KeyError(cfg["solver"])


class OracleFK:
    """Stand-in for capi.Context in CPU-only experiments/tests: workloads.make_batch only needs fk_batch().  segs: the oracle's chain
    (default: the Panda)."""

    def __init__(self, segs=None):
        self.segs = segs

    def fk_batch(self, desc, q):
        ch = orc.make_chain(self.segs or panda_segs())
        q = np.asarray(q, float)
        pos, quat = np.zeros((len(q), 3)), np.zeros((len(q), 4))
        for i in range(len(q)):
            pos[i], quat[i], *_ = orc.fk(ch, q[i])
        return pos, quat, None
