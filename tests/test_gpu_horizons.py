"""Every solver kernel at short and odd horizons against the oracle.

Each pipelined kernel walks the horizon through a prefetch ring of fixed depth, runs dummy steps where the step count is not a multiple of
it, and some store the last group's gain image in an epilogue.  A mistake there is wrong only at a few steps near t = 0 and only at the
horizons that reach it, so the horizons below cover every residue of every ring.  Which case reaches which kernel and residue:

  Riccati solvers (test_riccati_horizon), T = 2 .. 25: every residue modulo lcm(3, 4, 8) = 24 of T - 1 and T - 2, and every T below a ring
    C2   (PosOrn-1, uniform R: packed gain records) ILQR_FWD=dpp | wg   k_init_roll_lti (CH = 8, (T-1) mod 8),
         k_backward_si_dpp<fused, unif> (PF = 4, (T-2) mod 4, tail branch at (T-2) mod 4 = 3), k_forward_dpp (PF = 8, (T-1) mod 8) | k_forward_wg
         (8-step blocks, (T-1) mod 8)
    C2r  (joint-dependent R: plain records)          ILQR_FWD=dpp | wg   k_backward_si_dpp<..., unif = false>, the forward passes as C2
    C3   (PosOrn-1, AL)                              ILQR_FWD=dpp | wg   k_backward_si_dpp with an AL row, the forward passes as C2
    C1j  (JointSpace-1)                              default             k_backward_si_dpp on the joint-space system
    C2nd (PosOrn-2)                                  ILQR_SWEEP=mfma | rows   k_backward_mfma (PF = 3, (T-2) mod 3) | k_backward_rows (PF = 3,
         tail branch), k_forward_lin (PF = 4, (T-1) mod 4)
    C4t1, C4, C1t (time systems)  ILQR_SWEEP=mfma ILQR_APPLY=dpp | ILQR_SWEEP=rows ILQR_APPLY=rows   k_backward_mfma | k_backward_rows,
         k_forward_mfma (PF = 3, (T-1) mod 3), k_apply_dpp_tm | k_apply_rows_tm (PF = 3 / 4)
    C4al (AL on the matrix-core path)                default             the above with the AL update
  Generic kernels (test_riccati_generic), ILQR_HIP_PATH=v1, C2 and C4t1 at T in {2, 3, 5, 9, 17}: k_backward, k_forward
  Keypoint placements (test_riccati_keypoints), T in {17, 25}, keypoints at (0, T-1), (T-2, T-1), (7, 8), (8, 15): a keypoint at step 0, two
    in one 8-step block, a pair on both sides of a block boundary (k_forward_dpp's plain-block copy); C2 (ILQR_FWD=dpp | wg), C3, C4t1
  BatchILQRCP (test_batch_cp_horizon), C5-shaped (PosOrn-1, unit steps) and C4cp (time-2, sawtooth + unit-step sqrt(dt)) at
    T in {2, 3, 5, 9, 10, 17, 65, 66, 129}: k_cp_linearize (G = 4), k_cp_final (G = 8), k_cpl_states / k_cpl_final (CH = 8, 64-step basis
    tiles: T - 1 = 64 fills one tile exactly, 65 is one step past it, 128 is two tiles)
  BatchILQR at T = 65 and 66: tests/test_gpu_batchwide.py::test_batch_ilqr_edge_shapes.

A new ring depth d extends HORIZONS to lcm(24, d) + 1 (tests/horizons.py).  Every Riccati case is gated by tests/horizons.check_case: the
parity proof with instances 0 and 1 always proven, the gains at every step after 1 and 4 iterations, the trajectories where the path is the
oracle's.  The same horizons on the host build of the generic kernels: tests/test_horizons_cpu.py."""
import numpy as np
import pytest

from tests import horizons as hz
from tests.helpers import psi_of

pytestmark = pytest.mark.gpu

PINS = {  # kernel variants, through the environment as test_gpu_parity.py pins them (capi re-reads ILQR_* before every solve)
    "dpp": dict(ILQR_HIP_PATH="v2", ILQR_FWD="dpp"),
    "wg": dict(ILQR_HIP_PATH="v2", ILQR_FWD="wg"),
    "default": dict(ILQR_HIP_PATH="v2"),
    "mfma": dict(ILQR_HIP_PATH="v2", ILQR_SWEEP="mfma"),
    "rows": dict(ILQR_HIP_PATH="v2", ILQR_SWEEP="rows"),
    "mfma-dpp": dict(ILQR_HIP_PATH="v2", ILQR_SWEEP="mfma", ILQR_APPLY="dpp"),
    "rows-rows": dict(ILQR_HIP_PATH="v2", ILQR_SWEEP="rows", ILQR_APPLY="rows"),
    "v1": dict(ILQR_HIP_PATH="v1"),
}
RICCATI = [("C2", "dpp"), ("C2", "wg"), ("C2r", "dpp"), ("C2r", "wg"), ("C3", "dpp"), ("C3", "wg"), ("C1j", "default"), ("C2nd", "mfma"),
           ("C2nd", "rows")] + [(n, pin) for n in ("C4t1", "C4", "C1t") for pin in ("mfma-dpp", "rows-rows")] + [("C4al", "default")]
CP_HORIZONS = (2, 3, 5, 9, 10, 17, 65, 66, 129)


def _pin(monkeypatch, pin):
    for k in ("ILQR_HIP_PATH", "ILQR_SWEEP", "ILQR_FWD", "ILQR_APPLY", "ILQR_CP", "ILQR_CP_SOLVE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PINS[pin].items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def ctx():
    from ilqr_planner_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("T", hz.HORIZONS)
@pytest.mark.parametrize("name,pin", RICCATI, ids=[f"{n}-{p}" for n, p in RICCATI])
def test_riccati_horizon(ctx, monkeypatch, name, pin, T):
    _pin(monkeypatch, pin)
    cfg, desc, inp = hz.make_case(ctx, name, T)
    print(hz.check_case(ctx, cfg, desc, inp, f"{name} [{pin}] T={T}"))


@pytest.mark.parametrize("T", (2, 3, 5, 9, 17))
@pytest.mark.parametrize("name", ("C2", "C4t1"))
def test_riccati_generic(ctx, monkeypatch, name, T):
    _pin(monkeypatch, "v1")
    cfg, desc, inp = hz.make_case(ctx, name, T)
    print(hz.check_case(ctx, cfg, desc, inp, f"{name} [v1] T={T}"))


KP = [("C2", "dpp"), ("C2", "wg"), ("C3", "default"), ("C4t1", "default")]


@pytest.mark.parametrize("place", range(4))
@pytest.mark.parametrize("T", hz.KP_HORIZONS)
@pytest.mark.parametrize("name,pin", KP, ids=[f"{n}-{p}" for n, p in KP])
def test_riccati_keypoints(ctx, monkeypatch, name, pin, T, place):
    _pin(monkeypatch, pin)
    kp = hz.kp_placements(T)[place]
    cfg, desc, inp = hz.make_case(ctx, name, T, kp=kp)
    print(hz.check_case(ctx, cfg, desc, inp, f"{name} [{pin}] T={T} keypoints {kp}"))


@pytest.mark.parametrize("T", CP_HORIZONS)
@pytest.mark.parametrize("name", ("C5", "C4cp"))
def test_batch_cp_horizon(ctx, monkeypatch, name, T):
    """BatchILQRCP at its group, chunk and tile edges, with the configuration's basis cut to K <= T - 1 pieces; every instance has the
    oracle's step sizes and costs within 1e-4 of its end-to-end run or is proven iteration by iteration (tests/parity_proof.py), instances
    0 and 1 always; where the path is the oracle's, the controls agree too."""
    from ilqr_planner_amd import workloads
    from tests import parity_proof as pp

    _pin(monkeypatch, "default")
    cfg, desc, inp = hz.make_case(ctx, name, T)
    nb_iter = hz.NIT
    p = workloads.load_batch(ctx, desc, inp, hz.B)
    psi = psi_of(dict(cfg["psi"], K=min(cfg["psi"]["K"], T - 1)), T, p.dims.n_u)
    try:
        p.solve_batch_cp(psi, nb_iter, True)
        U = p.U()
        summ, rel, failures, runs = pp.check_batch_solver(p, cfg, inp, psi, nb_iter, True, lambda q, n, es: q.solve_batch_cp(psi, n, es))
    finally:
        p.close()
    print(f"{name} T={T} psi {psi.shape}: {summ}")
    assert not failures, f"{len(failures)} instance(s) neither within 1e-4 nor proven: {failures[:3]}"
    assert summ["frac_unexplained"] == 0.0 and summ["n_proven_always"] == 2, summ
    for i, r in runs.items():
        if rel[i] <= 1e-4 and np.all(np.isfinite(r["u"])):
            np.testing.assert_allclose(U[i].reshape(-1), r["u"], rtol=0, atol=1e-4 * max(1.0, np.abs(r["u"]).max()))
