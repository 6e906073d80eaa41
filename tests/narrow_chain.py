"""Chains of fewer than 7 joints (ilqr_planner_amd/csrc/ilqr_dofmap.hpp): cut Panda chains, oracle Systems at the native dof, and the same
problem written by hand as a 7-joint chain -- inert joints (zero axis, identity transform) inserted behind the last real joint, every per-joint
field and input widened field by field here, independently of the library's map."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import parity_proof as pp
from tests.helpers import orc, urdf_text
from ilqr_planner_amd import capi, workloads

D = 7
CHAINS = {6: "panda_link6", 3: "panda_link3"}  # tip frames of the cut chains of tests/golden/panda_chain.urdf


def capi_chain(dof):
    return capi.chain_from_urdf(urdf_text(), "panda_link0", CHAINS[dof])


def oracle_segs(dof):
    return orc.chain_from_urdf(urdf_text(), "panda_link0", CHAINS[dof])


def pad_chain(ch):
    """The chain with D - dof inert joints behind its last moving joint (works on capi and oracle chain dicts)."""
    dof = ch["dof"]
    last = max(i for i, j in enumerate(ch["seg_joint"]) if j >= 0)
    out = dict(ch)
    ins = dict(seg_joint=list(range(dof, D)), seg_xyz=[[0.0, 0.0, 0.0]] * (D - dof), seg_R=[[1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]] * (D - dof),
               seg_axis=[[0.0, 0.0, 0.0]] * (D - dof))
    for k, v in ins.items():
        seq = [list(e) if not isinstance(e, (int, np.integer)) else int(e) for e in ch[k]]
        out[k] = seq[: last + 1] + v + seq[last + 1:]
    for k in ("lower", "upper"):
        if k in ch:
            out[k] = np.concatenate([np.asarray(ch[k], float), np.zeros(D - dof)])
    out["dof"] = D
    return out


def maps(kind, nd, dof):
    """user index -> device index of the state and the control: joints keep theirs, velocities go to 7 + i, the time entry to the end"""
    tm = kind in (capi.SYS_POS_ORN_TIME, capi.SYS_JOINT_TIME)
    x = list(range(dof)) + ([D + i for i in range(dof)] if nd == 2 else []) + ([nd * D] if tm else [])
    u = list(range(dof)) + ([D] if tm else [])
    return np.array(x), np.array(u), nd * D + tm, D + tm


def widen_desc(d, chain7):
    """Descriptor d of a dof-joint problem written as the 7-joint problem: padded control weights = the first joint's, padded limits 0."""
    w = capi.ProblemDesc()
    C.memmove(C.byref(w), C.byref(d), C.sizeof(d))
    xm, um, nx7, nu7 = maps(d.kind, d.nb_deriv, d.dof)
    w.dof = D
    n = len(chain7["seg_joint"])
    w.n_seg = n
    for i in range(n):
        w.seg_joint[i] = int(chain7["seg_joint"][i])
        for k in range(3):
            w.seg_xyz[i][k] = float(chain7["seg_xyz"][i][k])
            w.seg_axis[i][k] = float(chain7["seg_axis"][i][k])
        for k in range(9):
            w.seg_R[i][k] = float(chain7["seg_R"][i][k])
    for k in range(d.n_kp):  # the n_x x n_x precision of a joint-space keypoint (hybrid sequence): padded rows and columns 0
        if d.kp_joint[k]:
            nx = len(xm)
            Q = np.array([d.kp_Q[k][i] for i in range(nx * nx)]).reshape(nx, nx)
            Q7 = np.zeros((nx7, nx7))
            Q7[np.ix_(xm, xm)] = Q
            for i, v in enumerate(Q7.reshape(-1)):
                w.kp_Q[k][i] = v
    inv_u = {int(j): i for i, j in enumerate(um)}
    for j in range(nu7):
        w.R_diag[j] = d.R_diag[inv_u.get(j, 0)]
        for k in range(d.n_kp):
            w.kp_Ru[k][j] = d.kp_Ru[k][inv_u.get(j, 0)]
    for f in ("state_max", "state_min", "limit_weight", "state_max2", "state_min2", "limit_weight2"):
        src, dst = getattr(d, f), getattr(w, f)
        vals = [src[i] for i in range(len(xm))]
        for j in range(len(dst)):
            dst[j] = 0
        for i, j in enumerate(xm):
            dst[int(j)] = vals[i]
    return w


def widen_inputs(inp, kind, nd, dof):
    xm, um, nx7, nu7 = maps(kind, nd, dof)
    B = inp["q0"].shape[0]
    out = dict(inp)
    out["q0"] = np.zeros((B, D))
    out["q0"][:, :dof] = inp["q0"]
    out["dq0"] = np.zeros((B, D))
    out["dq0"][:, :dof] = inp["dq0"]
    U0 = inp["U0"]
    out["U0"] = np.zeros(U0.shape[:2] + (nu7,))
    out["U0"][:, :, um] = U0
    if "A" in inp:
        nx = len(xm)
        A = np.zeros((inp["A"].shape[0], nx7 + nu7))
        A[:, xm] = inp["A"][:, :nx]
        A[:, nx7 + um] = inp["A"][:, nx:]
        out["A"] = A
    if "kp_joint" in inp:  # joint-space keypoint targets: the joint vector (+ time) in the first n_x of the n_f slots
        out["targets"] = list(inp["targets"])
        for k in inp["kp_joint"]:
            t = inp["targets"][k]
            t7 = np.zeros_like(t)
            t7[:, xm] = t[:, :len(xm)]
            out["targets"][k] = t7
    lim = inp["limits"]
    big = 10 * np.pi  # the oracle gives every state entry a limit weight of 1: inactive bounds on the inert joints
    smax, smin = np.full(nx7, big), np.full(nx7, -big)
    smax[xm], smin[xm] = lim["state_max"], lim["state_min"]
    out["limits"] = dict(state_max=smax, state_min=smin, limit_weight=np.ones(nx7, dtype=int))
    return out


def narrow_cfg(name, dof):
    cfg = workloads.config(name)
    if "al" in cfg and cfg["al"]["row"] >= dof:  # the tutorial's row q_6 <= 2 on a chain that has no q_6: the last joint
        cfg["al"] = dict(cfg["al"], row=dof - 1)
    if cfg.get("hybrid"):  # the joint-space via point's precision: its joints (+ the time entry, weighted here so that a time target in the
        q = cfg["Qdiag"][0]  # wrong slot shows)
        cfg["Qdiag"] = [list(q[:dof]) + ([0.1] if len(q) > D else [])] + list(cfg["Qdiag"][1:])
    return cfg


def make_pair(ctx, name, dof, B, seed=None):
    """(cfg, native desc, native inputs, 7-joint desc, 7-joint inputs) of one workload on the dof-joint cut Panda chain"""
    cfg = narrow_cfg(name, dof)
    ch = capi_chain(dof)
    desc, inp = workloads.make_batch(ctx, cfg, B=B, seed=seed, chain=ch)
    if cfg.get("hybrid"):  # the via point's target [q (, t)] fills the first n_x of its n_f = 7 (+ 1) slots; the rest is read by nothing
        nf = D + (1 if cfg["kind"] == capi.SYS_POS_ORN_TIME else 0)
        t = inp["targets"][0]
        inp["targets"][0] = np.hstack([t, np.zeros((t.shape[0], nf - t.shape[1]))])
        inp["kp_joint"] = [0]
    return cfg, desc, inp, widen_desc(desc, pad_chain(ch)), widen_inputs(inp, cfg["kind"], cfg["nb_deriv"], dof)


def oracle_system(cfg, inp, i, segs):
    """Oracle System of instance i of a make_batch batch on the chain segs (PosOrn kinds, no hybrid keypoints), at segs' dof."""
    dof = segs["dof"]
    nd, tm = cfg["nb_deriv"], cfg["kind"] == capi.SYS_POS_ORN_TIME
    kps = []
    for k, ts in enumerate(inp["kp_t"]):
        tg = inp["targets"][k][i]
        d = dict(timestep=ts, pos=tg[0:3], orn=tg[3:7], Q=np.diag(cfg["Qdiag"][k]))
        if nd == 2:
            d.update(dpos=tg[7:10], dorn=tg[10:14])
        if tm:
            d["ctime"] = tg[-1]
        kps.append(d)
    lim = inp["limits"]
    qMax, qMin = lim["state_max"][:dof], lim["state_min"][:dof]
    dqMax = lim["state_max"][dof:2 * dof] if nd == 2 else None
    dqMin = lim["state_min"][dof:2 * dof] if nd == 2 else None
    nu = dof + (1 if tm else 0)
    R = workloads.control_weights(cfg, nu)
    return orc.make_system(segs, orc.SYS_POS_ORN_TIME if tm else orc.SYS_POS_ORN, nd, cfg["T"], cfg["dt"], R, kps, inp["q0"][i][:dof],
                           inp["dq0"][i][:dof], qMax, qMin, dqMax, dqMin)


def oracle_solve(cfg, inp, i, segs, nb_iter, early_stop=True):
    s = oracle_system(cfg, inp, i, segs)
    U0 = inp["U0"][i].reshape(-1)
    if cfg["solver"] == "recursive":
        return orc.solve_recursive(s, U0, nb_iter, True, early_stop)
    al = cfg["al"]
    return orc.solve_al(s, inp["A"], inp["b"], inp["lambda0"][i], U0, nb_iter, al["lag"], al["penalty"], al["scaling"], True, early_stop)


def prove(cfg, inp, i, states, ct, at, iters, sysm):
    """Every iteration of instance i reproduced by one oracle iteration from the GPU's state (parity_proof's steps (b) and (c)), on the
    native chain's oracle System."""
    for it in range(int(iters[i])):
        r = pp.one_step(cfg, inp, i, it, states, sysm=sysm)
        pr = r["probe"][0]
        ok, _, why = pp.decisions_follow(pr, float(at[i, it]))
        if not ok:
            return f"iteration {it}: {why}"
        co = pp._cost_at(pr, float(at[i, it]))
        if co is None or pp._rel(float(ct[i, it]), co) > pp.STEP_RTOL:
            return f"iteration {it}: cost {ct[i, it]} vs {co}"
    return None


def results(p, nb_iter, gains=True):
    r = dict(X=p.X(), U=p.U(), cost=p.cost(), alpha=p.alpha(), trace=p.trace(nb_iter))
    if gains:
        r.update(K=p.K(), d=p.d())
    return r


def assert_embedded(nat, wide, kind, nd, dof):
    """Results of the native problem are the real entries of the 7-joint problem's, bit for bit; its padded entries are exactly 0 (on the
    instances whose solve stayed finite: a diverged one -- the reference prints -nan and carries on -- is NaN everywhere)."""
    xm, um, nx7, nu7 = maps(kind, nd, dof)
    xp, up = np.setdiff1d(np.arange(nx7), xm), np.setdiff1d(np.arange(nu7), um)
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)  # noqa: E731
    fin = np.isfinite(wide["cost"])
    assert same(nat["X"], wide["X"][:, :, xm])
    assert same(nat["U"], wide["U"][:, :, um])
    assert np.all(wide["X"][fin][:, :, xp] == 0) and np.all(wide["U"][fin][:, :, up] == 0)
    if "K" in nat:
        assert same(nat["K"], wide["K"][:, :, um][:, :, :, xm])
        assert same(nat["d"], wide["d"][:, :, um])
        assert np.all(wide["K"][fin][:, :, up, :] == 0) and np.all(wide["d"][fin][:, :, up] == 0)
    for k in ("cost", "alpha"):
        assert same(nat[k], wide[k]), k
    for a, b in zip(nat["trace"], wide["trace"]):
        assert same(a, b)
