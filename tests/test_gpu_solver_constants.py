"""The Riccati solvers away from the default reg, alpha_floor and stop_tol, on the device.

ilqr_problem_desc carries three constants a caller may set; every sweep, every forward pass with its decision kernel and the kernel plan read them.
The table of tests/solver_constants.py (its header says what each constant set reaches) runs a ragged batch of 13 at T = 14, 25 or 26 for 6
iterations:

  cooperative sets (n_alpha <= 16: floor 2^-3, 0.1, 4e-5; reg 1e-2, 0; stop_tol 1e-1, 1e-9)
      C2 [dpp, wg], C2r [dpp], C3 [dpp, wg], C1j       k_backward_si_dpp<FUSED = true>, k_forward_dpp | k_forward_reg with k_select, NA = 11 | 16
      C2nd [mfma, rows]                                k_backward_mfma | k_backward_rows, k_forward_lin<S, 11 | 16>
      C4t1, C4 [mfma-dpp, rows-rows], C4al             the same sweeps, k_forward_mfma with k_select_x, k_apply_dpp_tm | k_apply_rows_tm
      C2, C4t1 [v1]                                    the generic k_backward / k_forward
      C3 [wglds] at floor 4e-5                         k_forward_wg<16>
  sets past 16 step sizes (floor 2e-5, 1e-6; combined)
      C2, C2r, C3, C1j                                 k_backward_si_dpp<FUSED = false> (plain records), the generic k_forward; C3: Init::Lti,
                                                       k_al_post at it = -1, k_forward<AL = true>
      C3 with 4 binding state rows (al_shapes)         the same with MR = 4
      C2nd [mfma, rows], C4t1 [mfma-dpp, rows-rows], C4al   the cooperative sweeps under the generic forward pass

Gate of every case: horizons.check_case, as it stands -- the parity proof (tests/parity_proof.py, which takes the floor and the stop threshold from
the case) with instances 0 and 1 always proven, gains at every step after 1 and 6 iterations, trajectories where the path is the oracle's, every
multiplier update for AL; then the status words (solver_constants.check_case: the ALPHA_FLOOR bit exactly where the last line search ended at or below
the case's floor).  The reference is the oracle with the same constants (orc_set_constants).  That each case bites -- line searches that end
on both sides of the floor, gains that move by more than 100 tolerances with reg, iteration counts that change with stop_tol -- is asserted on the
oracle alone by tests/test_solver_constants_cpu.py, which also runs the [v1] cases on the host build of the generic kernels.  The one-line summaries
of a run are kept in profiles/solver_constants_parity.txt."""
import pytest

from tests import solver_constants as sc
from tests.test_gpu_horizons import PINS, _pin

pytestmark = pytest.mark.gpu

CASES = sc.cases()


@pytest.fixture(scope="module")
def ctx():
    from ilqr_planner_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("c", CASES, ids=[sc.case_id(c) for c in CASES])
def test_solver_constants(ctx, monkeypatch, c):
    if c["pin"] in PINS:
        _pin(monkeypatch, c["pin"])
    else:
        _pin(monkeypatch, "default")
        for k, v in sc.EXTRA_PINS[c["pin"]].items():
            monkeypatch.setenv(k, v)
    cfg, desc, inp = sc.make(ctx, c)
    print(sc.check_case(ctx, cfg, desc, inp, sc.case_id(c)))
