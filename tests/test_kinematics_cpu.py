"""Kinematics on chains that are not the Panda, on the CPU: the two URDF readers against each other and against their limits, the oracle's
FK, Jacobian and object-frame transform against the high-precision reference of tests/kinematics_reference.py (which first checks itself),
and the C ABI's folding of fixed segments and padding to seven joints (lower_chain, ilqr_dofmap.hpp) through the host build of the
lane-per-instance kernels.  The fixtures tests/golden/chains/gen7.urdf and gen4.urdf have what the Panda lacks: joint axes along x, y, -z and
oblique ones, origins with roll, pitch and yaw, fixed joints before, between (two in a row) and behind the moving ones.  The device side of
the same checks: tests/test_gpu_general_chain.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import kinematics_reference as kr
from tests.helpers import GENERAL_CHAINS, ROOT, TOOL_FRAMES, build_hostsim, general_chain, general_chain_text, object_frames, orc

HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")
CASES = [(n, t) for n in ("gen7", "gen4") for t in ("identity", "rotated")]
N = 300
ATOL = 1e-12  # the bound test_fk_batch_vs_oracle holds the device to


def _capi():
    from ilqr_planner_amd import capi

    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return capi


def _ref_chain(name):
    return kr.read_chain(general_chain_text(name), *GENERAL_CHAINS[name][1:])


def _tool(tool):
    rpy, xyz = TOOL_FRAMES[tool]
    return rpy or (0, 0, 0), xyz or (0, 0, 0)


@pytest.mark.parametrize("name,tool", CASES)
def test_reference_checks_itself(name, tool):
    """The analytic Jacobian of the reference against central differences of its own position and of R'(q) R^T, step 1e-15 in 50-digit
    arithmetic, and R R^T = I.  Measured disagreement of the Jacobian: 1.67e-31 on every chain and tool frame (the truncation term
    h^2 / 6 of a central difference of sines and cosines); the assertion is 100 times that.  Orthonormality: measured 1.4e-50, asserted
    at 1e-45 (a product of some twenty rotations, each orthonormal to the working precision of 1e-50)."""
    ref = _ref_chain(name)
    rng = np.random.default_rng(1)
    worst_j = worst_o = 0.0
    for _ in range(5):
        dj, do = kr.self_check(ref, rng.uniform(-3.1, 3.1, kr.dof_of(ref)), *_tool(tool))
        worst_j, worst_o = max(worst_j, dj), max(worst_o, do)
    print(f"reference self-check {name} {tool}: Jacobian vs central differences {worst_j:.3e}, orthonormality {worst_o:.3e}")
    assert worst_j <= 1.67e-29 and worst_o <= 1e-45


@pytest.mark.parametrize("name,tool", CASES + [("gen4cut3", "rotated")])
def test_readers_agree(name, tool):
    _capi()
    a, b = general_chain(name, tool)
    ref = _ref_chain(name)
    assert a["dof"] == b["dof"] == kr.dof_of(ref) == {"gen7": 7, "gen4": 4, "gen4cut3": 3}[name]
    assert a["seg_joint"] == b["seg_joint"] and len(a["seg_joint"]) == len(ref) + 1  # ... + the tool frame
    assert np.array_equal(np.array(a["seg_xyz"]), np.array(b["seg_xyz"]))
    np.testing.assert_allclose(a["seg_R"], b["seg_R"], rtol=0, atol=1e-16)
    mov = [i for i, j in enumerate(a["seg_joint"]) if j >= 0]
    ax = np.array(a["seg_axis"])[mov]
    assert np.array_equal(ax, np.array(b["seg_axis"])[mov])
    # unit length: the components and the norm each carry a rounding, two units in the last place of 1 in all
    assert np.all(np.abs(np.linalg.norm(ax, axis=1) - 1.0) <= 4.5e-16)
    assert np.array_equal(a["lower"], np.array(b["lower"])) and np.array_equal(a["upper"], np.array(b["upper"]))
    # ... and both say what the file says, read a third time
    mv = [j for j in ref if j["moving"]]
    np.testing.assert_allclose(ax, [[float(c) for c in j["axis"]] for j in mv], rtol=0, atol=2.3e-16)
    assert [float(j["lower"]) for j in mv] == list(a["lower"]) and [float(j["upper"]) for j in mv] == list(a["upper"])
    np.testing.assert_allclose(np.array(a["seg_xyz"])[:-1], [[float(c) for c in j["xyz"]] for j in ref], rtol=0, atol=0)
    for i, j in enumerate(ref):
        Rj = kr.Rz(j["rpy"][2]) * kr.Ry(j["rpy"][1]) * kr.Rx(j["rpy"][0])
        np.testing.assert_allclose(np.array(a["seg_R"][i]).reshape(3, 3), kr._np2(Rj), rtol=0, atol=4e-16)
    if name == "gen4":
        assert a["lower"][3] == -np.inf and a["upper"][3] == np.inf  # the continuous joint
        assert np.array_equal(ax[1], [1.0, 0.0, 0.0])  # the joint without <axis>
        assert np.isfinite(a["lower"][:3]).all() and np.isfinite(a["upper"][:3]).all()
    else:
        assert np.isfinite(a["lower"]).all() and np.isfinite(a["upper"]).all()


@pytest.mark.parametrize("name,tool", CASES)
def test_oracle_fk_vs_reference(name, tool):
    """orc.fk on N seeded configurations, uniform in +-3.1: position, signed quaternion, Jacobian, dx and w within 1e-12 absolute.
    Measured: 1.4e-15 at worst, no sample within 1e-9 of a branch boundary; branches (trace, R00, R11, R22) gen4 rotated 106 / 66 / 70 /
    58, gen7 rotated 112 / 56 / 48 / 84; every gen7 axis column has two components above 0.1 on at least 294 of 300 samples."""
    _, segs = general_chain(name, tool)
    oc, ref = orc.make_chain(segs), _ref_chain(name)
    dof = segs["dof"]
    rng = np.random.default_rng(7)
    q, dq = rng.uniform(-3.1, 3.1, (N, dof)), rng.uniform(-1.0, 1.0, (N, dof))
    branches, near, worst, two = [0] * 4, 0, 0.0, np.zeros(dof, dtype=int)
    for i in range(N):
        r = kr.fk(ref, q[i], *_tool(tool), dq=dq[i])
        p, qt, J, dx, w = orc.fk(oc, q[i], dq[i])
        near += kr.assert_pose(r, p, qt, J, atol=ATOL, what=(name, tool, i))
        assert np.max(np.abs(dx - r["dx"])) <= ATOL and np.max(np.abs(w - r["w"])) <= ATOL, (name, tool, i)
        np.testing.assert_allclose(np.concatenate([dx, w]), r["J"] @ dq[i], rtol=0, atol=ATOL)
        worst = max(worst, np.abs(p - r["pos"]).max(), np.abs(J - r["J"]).max(), np.abs(dx - r["dx"]).max(), np.abs(w - r["w"]).max())
        branches[r["branch"]] += 1
        two += (np.abs(r["J"][3:]) > 0.1).sum(axis=0) >= 2
    print(f"oracle FK {name} {tool}: worst deviation {worst:.2e}; branches {branches}; {near} of {N} compared up to sign; "
          f"axis columns with two components above 0.1: {two.tolist()}")
    assert near <= 0.02 * N
    if (name, tool) == ("gen4", "rotated"):
        assert min(branches) >= 20, branches
    if name == "gen7":
        assert np.all(two >= N // 2), two


@pytest.mark.parametrize("which", [0, 1])
def test_oracle_object_frame_vs_reference(which):
    """The oracle's pose and Jacobian as seen from an object frame (TransformedSimulationInterface) on gen7, against the reference with
    Eigen's sign rule restated: trace > 0, else the largest diagonal entry.  Measured: 35 and 37 of 64 samples off the trace branch, none
    within 1e-9 of a boundary."""
    T = object_frames()[which]
    _, segs = general_chain("gen7", "rotated")
    ref = _ref_chain("gen7")
    kp = dict(timestep=1, pos=[0, 0, 0], orn=[1, 0, 0, 0], Q=np.eye(6), frame=T)
    s = orc.make_system(segs, orc.SYS_POS_ORN, 1, 2, 0.1, [1e-5] * 7, [kp], [0.0] * 7)
    n, off, near = 64, 0, 0
    q = np.random.default_rng(11).uniform(-3.1, 3.1, (n, 7))
    for i in range(n):
        r = kr.fk(ref, q[i], *_tool("rotated"), frame=(T[:3, :3], T[:3, 3]))
        fx, J = orc.get_fx_jac(s, q[i], kp=0)
        near += kr.assert_pose(r, fx[:3], fx[3:7], J, atol=ATOL, what=(which, i))
        off += r["branch"] != 0
    print(f"oracle object frame {which}: {off} of {n} off the trace branch, {near} compared up to sign")
    assert off >= 5 and near <= 0.02 * n


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory):
    return build_hostsim(tmp_path_factory.mktemp("hostsim") / "libilqr_hostsim.so")


def test_lower_chain_on_host_build(hostsim):
    """ilqr_fk_batch of the C ABI, built for the host, on gen7, gen4 and gen4 cut behind its third joint with both tool frames, against
    the reference at 1e-12: the folding of fixed segments into the next joint's pre-transform (before the first joint, two in a row
    between joints, behind the last) and the padding of three and four joints to seven behind axes that are not z."""
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "narrow_chain_checks.py"), hostsim, "general"], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "general chains: ok"


# ---- the reader's limits and errors


def _synth(types, extra=""):
    """A straight chain s0 -> s1 -> ... of joints of the given types, every origin and axis general."""
    out = ["<robot name='synth'>"]
    for i, t in enumerate(types):
        lim = "<limit lower='-2' upper='2'/>" if t in ("revolute", "prismatic") else ""
        ax = f"<axis xyz='{1 + i % 3} {(i % 2) - 1} {2 - i % 4}'/>" if t != "fixed" else ""
        out.append(f"<joint name='sj{i}' type='{t}'><parent link='s{i}'/><child link='s{i + 1}'/>"
                   f"<origin xyz='0.0{1 + i % 7} -0.0{1 + i % 5} 0.0{2 + i % 4}' rpy='0.{1 + i % 8} -0.{2 + i % 6} 0.{3 + i % 5}'/>{ax}{lim}</joint>")
    return "\n".join(out + [extra, "</robot>"])


def test_reader_limits_and_errors():
    capi = _capi()
    max_seg = capi.MAX_SEG
    assert max_seg == orc.MAX_SEG == 24
    types = ["fixed", "revolute", "fixed"] * 7 + ["fixed", "fixed"]  # 23 joints, 7 of them moving
    assert len(types) == max_seg - 1
    tool = TOOL_FRAMES["rotated"]
    a = capi.chain_from_urdf(_synth(types), "s0", f"s{len(types)}", *tool)
    b = orc.chain_from_urdf(_synth(types), "s0", f"s{len(types)}", *tool)
    assert a["dof"] == b["dof"] == 7 and len(a["seg_joint"]) == max_seg and a["seg_joint"] == b["seg_joint"]
    np.testing.assert_allclose(a["seg_R"], b["seg_R"], rtol=0, atol=1e-16)
    oc, ref = orc.make_chain(b), kr.read_chain(_synth(types), "s0", f"s{len(types)}")
    for q in np.random.default_rng(2).uniform(-3.1, 3.1, (3, 7)):  # the longest chain that loads is also evaluated right
        p, qt, J, _, _ = orc.fk(oc, q)
        kr.assert_pose(kr.fk(ref, q, *tool), p, qt, J, atol=ATOL)
    with pytest.raises(RuntimeError, match="too many segments"):
        capi.chain_from_urdf(_synth(types + ["fixed"]), "s0", f"s{len(types) + 1}", *tool)
    with pytest.raises(RuntimeError, match=r"prismatic.*sj2"):
        capi.chain_from_urdf(_synth(["revolute", "fixed", "prismatic", "revolute"]), "s0", "s4")
    with pytest.raises(RuntimeError, match=r"zero axis.*sj1"):
        capi.chain_from_urdf(_synth(["revolute", "revolute"]).replace("<axis xyz='2 0 1'/>", "<axis xyz='0 0 0.0'/>"), "s0", "s2")
    # a prismatic joint on a branch that does not lead to the tip is not looked at
    side = "<joint name='side' type='prismatic'><parent link='s1'/><child link='gripper'/><axis xyz='0 0 0'/></joint>"
    plain = capi.chain_from_urdf(_synth(["revolute", "fixed", "revolute"]), "s0", "s3")
    branched = capi.chain_from_urdf(_synth(["revolute", "fixed", "revolute"], side), "s0", "s3")
    assert plain["dof"] == branched["dof"] == 2
    for k in ("seg_joint", "seg_xyz", "seg_R", "seg_axis"):
        assert plain[k] == branched[k]
    assert np.array_equal(plain["lower"], branched["lower"]) and np.array_equal(plain["upper"], branched["upper"])
