"""Chains of 6 and 3 joints through the C ABI on the host build of the lane-per-instance kernels (tests/test_narrow_chain_cpu.py builds the
library and runs this script in a child process of its own: its library never meets the product library).

    python tests/tools/hostsim/narrow_chain_checks.py <libilqr_hostsim.so>
    python tests/tools/hostsim/narrow_chain_checks.py <libilqr_hostsim.so> general

"general": instead, FK and the Jacobian of the hand-written chains of tests/golden/chains/ (fixed segments folded before, between and behind
the joints; four joints padded to seven behind axes that are not z) with both tool frames, against tests/kinematics_reference.py.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ilqr_planner_amd import capi, workloads  # noqa: E402

capi.LIB_PATH = sys.argv[1]  # the host build, not the product library
os.environ["ILQR_HIP_PATH"] = "v1"  # every solve of capi.BatchProblem re-applies the cross-check switches of the environment

from tests import narrow_chain as nc  # noqa: E402
from tests.helpers import orc  # noqa: E402

B, NIT = 3, 6
SHAPES = (("C2", "C3"), ("C2nd", "C2ndal"), ("C4t1", "C4t1al"), ("C4", "C4al"))  # (recursive, AL) of POS_ORN 1, 2 and POS_ORN_TIME 1, 2


def check_fk(ctx, dof, chain=None):
    """chain = (name, tool) of tests.helpers.GENERAL_CHAINS / TOOL_FRAMES: that chain against the high-precision reference; None: the cut
    Panda chain of dof joints against the oracle."""
    if chain is not None:
        return check_fk_general(ctx, dof, *chain)
    ch = nc.capi_chain(dof)
    assert ch["dof"] == dof
    desc = capi.make_desc(kind=capi.SYS_POS_ORN, nb_deriv=1, horizon=2, dt=0.1, R_diag=[1e-5] * dof, chain=ch, kp_timesteps=[], kp_Q=[])
    q = np.random.default_rng(dof).uniform(ch["lower"], ch["upper"], (5, dof))
    pos, quat, jac = ctx.fk_batch(desc, q)
    oc = orc.make_chain(nc.oracle_segs(dof))
    for i in range(len(q)):
        p, qt, J, *_ = orc.fk(oc, q[i])
        assert np.allclose(pos[i], p, atol=1e-12, rtol=0) and np.allclose(quat[i], qt, atol=1e-12, rtol=0), (dof, i)
        assert jac[i].shape == (6, dof) and np.allclose(jac[i], J, atol=1e-12, rtol=0), (dof, i)
    print(f"fk {dof} joints: pose and Jacobian match the oracle", flush=True)


def check_fk_general(ctx, dof, name, tool, n=40):
    from tests import kinematics_reference as kr
    from tests.helpers import GENERAL_CHAINS, TOOL_FRAMES, general_chain, general_chain_text

    ch, _ = general_chain(name, tool)
    assert ch["dof"] == dof
    desc = capi.make_desc(kind=capi.SYS_POS_ORN, nb_deriv=1, horizon=2, dt=0.1, R_diag=[1e-5] * dof, chain=ch, kp_timesteps=[], kp_Q=[])
    q = np.random.default_rng(100 + dof).uniform(-3.1, 3.1, (n, dof))
    pos, quat, jac = ctx.fk_batch(desc, q)
    ref = kr.read_chain(general_chain_text(name), *GENERAL_CHAINS[name][1:])
    rpy, xyz = TOOL_FRAMES[tool]
    near = 0
    for i in range(n):
        r = kr.fk(ref, q[i], rpy or (0, 0, 0), xyz or (0, 0, 0))
        near += kr.assert_pose(r, pos[i], quat[i], jac[i], atol=1e-12, what=(name, tool, i))
    assert near <= 0.02 * n, (name, tool, near)
    print(f"fk {name} ({dof} joints, {tool} tool): pose and Jacobian match the high-precision reference; {near} of {n} at a branch boundary", flush=True)


def check_solves(ctx, dof):
    segs, segs7 = nc.oracle_segs(dof), nc.pad_chain(nc.oracle_segs(dof))
    for pair in SHAPES:
        for name in pair:
            cfg, desc, inp, desc7, inp7 = nc.make_pair(ctx, name, dof, B)
            p = workloads.load_batch(ctx, desc, inp, B)
            workloads.run_solver(p, cfg, nb_iter=NIT, early_stop=True)
            nat = nc.results(p, NIT)
            p.close()
            p7 = workloads.load_batch(ctx, desc7, inp7, B)
            workloads.run_solver(p7, cfg, nb_iter=NIT, early_stop=True)
            wide = nc.results(p7, NIT)
            p7.close()
            nc.assert_embedded(nat, wide, cfg["kind"], cfg["nb_deriv"], dof)
            ct, at = nat["trace"]
            for i in range(B):
                r = nc.oracle_solve(cfg, inp, i, segs, NIT)
                r7 = nc.oracle_solve(cfg, inp7, i, segs7, NIT)
                n = r["iters"]
                # the oracle agrees with itself on the native and the hand-padded chain
                assert r7["iters"] == n and np.array_equal(r7["trace_alpha"], r["trace_alpha"]), (name, dof, i)
                assert np.allclose(r7["trace_cost"], r["trace_cost"], rtol=1e-12, atol=0, equal_nan=True), (name, dof, i)
                # the device path against the oracle at the native dof: step sizes exactly, costs to rounding
                assert np.array_equal(at[i, :n], r["trace_alpha"]), (name, dof, i, at[i, :n], r["trace_alpha"])
                assert np.allclose(ct[i, :n], r["trace_cost"], rtol=1e-9, atol=0, equal_nan=True), (name, dof, i, ct[i, :n], r["trace_cost"])
                assert np.all(np.isnan(ct[i, n:])), (name, dof, i)
                assert np.allclose(nat["cost"][i], r["cost"], rtol=1e-9, atol=0, equal_nan=True), (name, dof, i)
            print(f"{name} {dof} joints: exact embedding, oracle traces, oracle self-agreement", flush=True)


def check_hybrid(ctx, dof):
    """Hybrid sequences (a joint-space via point of a JointSpace(Time)PlannerSys sub-system, kp_joint): the target map and the n_x x n_x
    precision widening, pinned by the exact embedding (the oracle's test helpers build these only for 7 joints)."""
    for name in ("C2h", "C4h", "C2hl"):
        cfg, desc, inp, desc7, inp7 = nc.make_pair(ctx, name, dof, B)
        res = []
        for d, i in ((desc, inp), (desc7, inp7)):
            p = workloads.load_batch(ctx, d, i, B)
            workloads.run_solver(p, cfg, nb_iter=NIT, early_stop=False)
            res.append(nc.results(p, NIT))
            p.close()
        nc.assert_embedded(res[0], res[1], cfg["kind"], cfg["nb_deriv"], dof)
        assert np.isfinite(res[0]["cost"]).all()
        print(f"{name} {dof} joints: exact embedding", flush=True)


def check_errors(ctx):
    ch = nc.capi_chain(6)
    for dof, chain in ((0, dict(ch, dof=0)), (8, dict(ch, dof=8)), (5, dict(ch, dof=5))):
        desc = capi.make_desc(kind=capi.SYS_POS_ORN, nb_deriv=1, horizon=10, dt=0.1, R_diag=[1e-5] * 8, chain=chain, kp_timesteps=[], kp_Q=[])
        try:
            capi.BatchProblem(ctx, desc, 2)
        except RuntimeError as e:
            assert "1 to 7 moving joints" in str(e), str(e)
            if dof == 5:
                assert "chain has 6 moving joints, descriptor says 5" in str(e), str(e)
        else:
            raise AssertionError(f"dof = {dof} was accepted")
    print("errors: dof 0, dof 8 and a chain / dof mismatch are refused with the allowed range", flush=True)


def main():
    ctx = capi.Context(0)
    ctx.set_crosscheck(generic_kernels=True)
    if sys.argv[2:] == ["general"]:
        for name, dof in (("gen7", 7), ("gen4", 4), ("gen4cut3", 3)):
            for tool in ("identity", "rotated"):
                check_fk(ctx, dof, chain=(name, tool))
        ctx.close()
        print("general chains: ok")
        return
    check_errors(ctx)
    for dof in (6, 3):
        check_fk(ctx, dof)
        check_solves(ctx, dof)
        check_hybrid(ctx, dof)
    ctx.close()
    print("narrow chains: ok")


if __name__ == "__main__":
    main()
