"""AL-iLQR sweeps at every constraint-row capacity, multipliers included.

The number of inequality rows m decides which sweep runs and how it holds the rows (csrc/ilqr_plan.hpp): up to 4 shared state-only rows in the
registers of k_backward_si_dpp (launch_dpp2: per-row offsets, a ring of PF x MR multipliers, rows rr >= m clamped to row 0), up to 16 rows in the
LDS of k_backward_mfma (slam[16], sIs[16]) or one per lane of an instance's 16-lane group in k_backward_rows, and everything else in the generic
k_backward with its workspace under the cooperative forward pass and k_al_post.  The workloads carry one row; the constraint sets of
tests/al_shapes.py bind for part of a ragged batch of 13 on positions, velocities, the time state and the controls.  Which case reaches what:

  test_register_rows            k_backward_si_dpp with m = 1 .. 4: C3 (PosOrn-1) under ILQR_FWD=dpp | wg, C3 with joint-dependent control weights (the
                                general sweep form, plain gain records), C1jal (JointSpace-1); unit rows, a dense row at m = 2 and 4; T = 25 (T = 40 with all
                                four rows in use: tests/test_gpu_fullsize.py::test_sweep_lane_groupings_agree)
  test_register_rows_overflow   one past it and its other ways out: m = 5, control rows, one set per step -- PosOrn-1 goes to k_backward_mfma,
                                JointSpace-1 to the generic sweep under k_forward_dpp
  test_lds_rows                 k_backward_mfma | k_backward_rows with m = 2, 15, 16 on C2ndal (rows 7 .. 13 on the velocities), C4t1al, C4al, C1tal (a
                                row on the time state; with `control` a lower bound on the time control), C3 at 15 and 16
  test_lds_rows_overflow        m = 17 and 32 (the oracle's ORC_MAX_M): the generic sweep and its workspace under the cooperative forward passes and
                                k_al_post (default), and the generic kernels throughout (v1)
  test_rows_at_ring_residues    the prefetch rings with a full set of rows: m = 4 on k_backward_si_dpp (PF = 4), m = 16 on k_backward_rows and
                                k_backward_mfma (PF = 3) at T = 2 .. 14 -- without C2ndal and C4al at T = 2, where the rows cannot bind (the only step is
                                k = 0 and every velocity is zero there: al_shapes.RESIDUE_DROPPED, tests/test_al_shapes_cpu.py)
  test_generic_pin              k_backward / k_forward with m = 4 and 16, dense rows

Gate of every case, al_shapes.check_case: the rows bind on the oracle's solve (tests/test_al_shapes_cpu.py asserts it for this whole table without a
GPU); horizons.check_case with 6 iterations and an update every 2 -- the parity proof with instances 0 and 1 always proven, which recomputes
every multiplier update from the device's own trajectory in extended precision and requires the multipliers not to move by a bit between updates
(parity_proof.check_multipliers), gains at every step after 1 and 6 iterations, trajectories where the path is the oracle's; and the multipliers
after the solve against the oracle's on those instances.

k_backward_si_dpp<FUSED = false> runs only with alpha_floor < 2^-15 (the generic forward pass): tests/test_gpu_solver_constants.py, with MR = 1 and
with the 4-row state-only set of this table.  The same sets on the host build of the generic kernels: tests/test_al_shapes_cpu.py."""
import pytest

from tests import al_shapes as al
from tests.test_gpu_horizons import _pin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from ilqr_planner_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


def _run(ctx, monkeypatch, c):
    _pin(monkeypatch, c["pin"])
    cfg, desc, inp = al.make(ctx, c)
    print(al.check_case(ctx, cfg, desc, inp, al.case_id(c)))


def _params(test):
    cs = al.cases(test)
    return pytest.mark.parametrize("c", cs, ids=[al.case_id(c) for c in cs])


@_params("register_rows")
def test_register_rows(ctx, monkeypatch, c):
    _run(ctx, monkeypatch, c)


@_params("register_rows_overflow")
def test_register_rows_overflow(ctx, monkeypatch, c):
    _run(ctx, monkeypatch, c)


@_params("lds_rows")
def test_lds_rows(ctx, monkeypatch, c):
    _run(ctx, monkeypatch, c)


@_params("lds_rows_overflow")
def test_lds_rows_overflow(ctx, monkeypatch, c):
    _run(ctx, monkeypatch, c)


@_params("rows_at_ring_residues")
def test_rows_at_ring_residues(ctx, monkeypatch, c):
    _run(ctx, monkeypatch, c)


@_params("generic_pin")
def test_generic_pin(ctx, monkeypatch, c):
    _run(ctx, monkeypatch, c)
