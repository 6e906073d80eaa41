"""Multi-start solves on the device (ilqr_problem_adopt, ilqr_problem_spread_controls, ilqr_problem_select, ilqr_problem_get_at): k_adopt_rows,
k_spread_controls, k_select_group in its forms of 1, 4, 16 and 64 lanes per group and k_get_at, held to the checks of tests/multistart.py, with the
_dev forms on torch tensors.  The systems at T = 2, 3, 9; the groups of the host build, (3, 64), (2, 65) and (128, 16).  At B = 2048 select, get_at and
adopt run on plans solved as two halves on two streams (tests/multistart.SPLIT_CASES: C4, which AUTO splits there, and C3 under
ilqr_ctx_set_split(2), which AUTO does not), so that a split plan's halves are selected from, read and adopted from.  adopt runs under AUTO and under the generic pin;
the planted-winner pipeline under the generic pin (the coarse solve runs on G * S instances, the direct one on G: only fixed pins give one
instance the same bytes in both).  The class level: solve_multistart of PyLQR against the same sequence through capi.py.
The host build of the generic kernels: tests/test_multistart_cpu.py."""
import os
import sys

import numpy as np
import pytest

from ilqr_planner_amd import capi
from tests import closed_loop as cl
from tests import multistart as ms
from tests.helpers import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

ALL_GROUPS = ms.GROUPS + ms.GROUPS_DEVICE + (ms.BIG,)


class TorchArrays:
    """The arrays of a _dev call: torch tensors on the device (the library runs on its own stream: callers synchronise the context before get)."""

    def put(self, a):
        import torch

        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        torch.cuda.synchronize()
        return t

    def empty(self, shape, dtype=np.float64):
        import torch

        t = torch.zeros(shape, dtype=torch.float64 if dtype == np.float64 else torch.int32, device="cuda")
        torch.cuda.synchronize()
        return t

    def ptr(self, h):
        return h.data_ptr()

    def get(self, h):
        return h.cpu().numpy()


@pytest.fixture(scope="module")
def ctx():
    import torch

    torch.cuda.init()  # torch's device first, then the library's context (the _dev forms are handed torch tensors)
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def arrays():
    return TorchArrays()


@pytest.mark.parametrize("G,S", ALL_GROUPS)
def test_select_every_group_shape(ctx, arrays, G, S):
    ms.check_select(ctx, arrays, "C3", 3, G, S, f"C3 T=3 G={G} S={S}")


@pytest.mark.parametrize("T", ms.HORIZONS)
@pytest.mark.parametrize("name", ms.SYSTEMS)
def test_select_every_system(ctx, arrays, name, T):
    ms.check_select(ctx, arrays, name, T, 5, 3, f"{name} T={T} G=5 S=3")


class _split:
    """The context's two-stream mode for the calls inside (None: the default, 1), put back afterwards."""

    def __init__(self, ctx, mode):
        self.ctx, self.mode = ctx, mode

    def __enter__(self):
        if self.mode is not None:
            self.ctx.set_split(self.mode)

    def __exit__(self, *a):
        if self.mode is not None:
            self.ctx.set_split(1)
        return False


@pytest.mark.parametrize("name,mode", ms.SPLIT_CASES)
def test_select_after_a_split_solve(ctx, arrays, name, mode):
    G, S = ms.BIG
    with _split(ctx, mode):
        ms.check_select(ctx, arrays, name, 9, G, S, f"{name} T=9 G={G} S={S} split={mode}")


@pytest.mark.parametrize("T", ms.HORIZONS)
@pytest.mark.parametrize("name", ms.SYSTEMS)
def test_get_at(ctx, arrays, name, T):
    ms.check_get_at(ctx, arrays, name, T, 13, f"{name} T={T}")


@pytest.mark.parametrize("name,mode", ms.SPLIT_CASES)
def test_get_at_of_a_split_plan(ctx, arrays, name, mode):
    with _split(ctx, mode):
        ms.check_get_at(ctx, arrays, name, 9, ms.BIG[0] * ms.BIG[1], f"{name} T=9 B=2048 split={mode}")


@pytest.mark.parametrize("pin", [None, "generic"])
@pytest.mark.parametrize("T", ms.HORIZONS)
@pytest.mark.parametrize("name", ms.SYSTEMS)
def test_adopt(ctx, arrays, name, T, pin):
    with (cl.generic_pin() if pin else _no_pin()):
        ms.check_adopt(ctx, arrays, name, T, 13, 15, f"{name} T={T} {pin} adopt 13 <- 15")
        ms.check_adopt(ctx, arrays, name, T, 70, 5, f"{name} T={T} {pin} adopt_dev 70 <- 5", dev_form=True)


@pytest.mark.parametrize("name,mode", ms.SPLIT_CASES)
def test_adopt_from_a_split_plan(ctx, arrays, name, mode):
    B = ms.BIG[0] * ms.BIG[1]
    with _split(ctx, mode):
        ms.check_adopt(ctx, arrays, name, 9, B, B, f"{name} T=9 adopt_dev 2048 <- 2048 split={mode}", dev_form=True)


def test_adopt_refusals_and_clamp(ctx, arrays):
    ms.check_adopt_refusals(ctx, "refusals")
    ms.check_adopt_dev_clamps(ctx, arrays, "clamp")


@pytest.mark.parametrize("T", ms.HORIZONS)
@pytest.mark.parametrize("name", ms.SYSTEMS)
def test_spread(ctx, name, T):
    for G, S in ((5, 3), (1, 70)):
        ms.check_spread(ctx, name, T, G, S, f"{name} T={T} G={G} S={S}")


@pytest.mark.parametrize("G,S", ((13, 1),) + ms.GROUPS_DEVICE + (ms.BIG,))
def test_spread_every_group_shape(ctx, G, S):
    ms.check_spread(ctx, "C4", 3, G, S, f"C4 T=3 G={G} S={S}")


@pytest.mark.parametrize("S", (3, 64))
@pytest.mark.parametrize("name", ms.PIPELINE)
def test_pipeline_picks_the_planted_winner(ctx, arrays, name, S):
    with cl.generic_pin():
        cfg, desc, inp, Uconv = ms.planted(ctx, name, 9, 5)
        ms.check_planted_condition(name, cfg, inp, Uconv, f"{name} planted")
        ms.check_pipeline(ctx, arrays, cfg, desc, inp, Uconv, S, f"{name} pipeline G=5 S={S}")


class _no_pin:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


# ---- (f) the class level

def _pylqr_solver(cfg, inp, T, al):
    sys.path.insert(0, os.path.join(ROOT, "ilqr_planner_amd", "pylqr"))
    from PyLQR.sim import KDLRobot
    from PyLQR.solver import AL_ILQR, Constraint, ILQRRecursive
    from PyLQR.system import PosOrnKeypoint, PosOrnPlannerSys
    from ilqr_planner_amd import workloads

    qMax = np.full(7, 10 * np.pi)
    rbt = KDLRobot(os.path.join(GOLDEN, "panda_chain.urdf"), "panda_link0", "panda_tip", list(inp["q0"][0]), [0.0] * 7)
    kps = [PosOrnKeypoint(np.array(tg[0][0:3]), np.array(tg[0][3:7]), np.diag(cfg["Qdiag"][k]), int(inp["kp_t"][k])) for k, tg in enumerate(inp["targets"])]
    sys_ = PosOrnPlannerSys(rbt, kps, list(workloads.control_weights(cfg, 7)), qMax, -qMax, T, 1, cfg["dt"])
    if not al:
        return ILQRRecursive(sys_)
    cons = []
    for _ in range(T - 1):
        c = Constraint()
        c.A, c.b = inp["A"], inp["b"]
        cons.append(c)
    return AL_ILQR(sys_, cons, [inp["lambda0"][0, k] for k in range(T - 1)])


@pytest.mark.parametrize("al", [False, True])
def test_solve_multistart_is_the_sequence_by_hand(ctx, al):
    T, G, S, seed, coarse, nit = 9, 5, 6, 4711, 2, 3
    cfg, desc, inp = ms.make_case(ctx, "C3", T, G)
    if not al:
        cfg = {k: v for k, v in cfg.items() if k != "al"}
        inp = {k: v for k, v in inp.items() if k not in ("A", "b", "lambda0")}
    sigma = ms.sigma_u(7, 0.3)
    a = cfg.get("al")
    pre = (inp["U0"], nit, a["lag"], a["penalty"], a["scaling"], True, False) if al else (inp["U0"], nit, True, False)
    common = dict(q0=inp["q0"], kp_targets=list(inp["targets"]))
    kept = ("X", "U", "cost", "alpha", "iters", "status")
    got = _pylqr_solver(cfg, inp, T, al).solve_multistart(*pre, S=S, seed=seed, sigma_u=sigma, coarse_iter=coarse, **common)
    ref, sel, first = ms.multistart_by_hand(ctx, cfg, desc, inp, S, seed, sigma, coarse, nit)
    for f in kept:
        assert np.asarray(getattr(got, f)).tobytes() == ref[f].astype(np.asarray(getattr(got, f)).dtype).tobytes(), f"solve_multistart: {f} differs from the sequence by hand"
    assert np.array_equal(got.winner, sel.winner) and np.array_equal(got.n_candidates, sel.n_candidates)
    assert got.coarse_best.tobytes() == sel.best.tobytes() and got.coarse_first.tobytes() == first.tobytes()
    assert np.all(got.coarse_best <= got.coarse_first)
    assert np.any(got.winner % S != 0), "no start but member 0 ever won: the spread did nothing"
    # S = 1, sigma_u = 0: a solve of coarse_iter iterations continued from its own plan
    one = _pylqr_solver(cfg, inp, T, al).solve_multistart(*pre, S=1, coarse_iter=coarse, **common)
    cont = ms.continued_by_hand(ctx, cfg, desc, inp, coarse, nit)
    for f in kept:
        assert np.asarray(getattr(one, f)).tobytes() == cont[f].astype(np.asarray(getattr(one, f)).dtype).tobytes(), f"solve_multistart(S=1): {f} differs"
    assert np.array_equal(one.winner, np.arange(G)) and one.coarse_best.tobytes() == one.coarse_first.tobytes()
