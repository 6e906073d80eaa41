"""Batched closed-loop rollouts of the tracking law (ilqr_problem_closed_loop) -- cases and checks shared by
tests/tools/hostsim/closed_loop_checks.py (the host build of the generic kernel) and tests/test_gpu_closed_loop.py (the device kernels).

The reference has no such call: it is the replay loop of its tutorials, so the check is that loop in NumPy on the arrays the getters return,
with the oracle's own step and cost:
  (a) X, U against the replay: per step within 1e-9 max(1, |x_k|_inf) (|u_k|_inf for U), the figures of test_gpu_fullsize for "X is the
      rollout of U";
  (b) J against the sum of orc.cost along the replayed trajectory, 1e-9 relative;
  (c) U[b][s][k] == p.track(k, X[b][s][k], ff) within (a)'s bound, for both ff;
  (d) x0 = None, w = None, no feed-forward: X is p.X() within (a)'s bound, J is p.cost() to 1e-9 relative after solve_recursive, and S copies
      of the one sample are bit-identical.
A closed loop multiplies rounding by its gains at every step.  Where a sample misses (a) or (b), the project's rule for ill-conditioned cases
applies in place of a wider constant: its deviation may be at most ILL_FACTOR times what the replay itself moves when its gain product is
accumulated in np.longdouble instead of float64.  Such samples are counted and the worst ratio reported."""
from __future__ import annotations

import contextlib
import os

import numpy as np

from ilqr_planner_amd import workloads
from tests import horizons as hz
from tests import narrow_chain as nc
from tests import shared_steps as ss
from tests.helpers import oracle_system_of_instance, orc

SHAPES = ("C2", "C2r", "C3", "C2nd", "C4t1", "C4", "C1j", "C1t", "C2h", "C2hl")
EXTRA = ("chain3", "shared", "limits")   # a 3-joint chain, keypoints that share a step, joint limits that bind
B = 13          # ragged: no multiple of the 1 .. 16 instances a wave holds
NIT = 3         # iterations of the solve that makes the plan
# The time systems (dt = u_last^2) start far from a plan: after a few iterations the feed-forward is still of the size of the controls, and the loop
# closed around such a plan leaves every bound within a dozen steps for some of the 13 x 65 executions (on the 2nd-order one, C4, at T >= 17 for
# most batches at any iteration count).  Their plans get NIT_TIME iterations, and the batch seed of every (shape, T) is the first of 1, 2, .. for
# which the replay of every sample used here (both ff) stays finite and bounded (1e3; C4 at T = 17, 25: 1e5, with the iteration count given) --
# found on the host build of the generic kernel; every check asserts the finiteness again.
NIT_TIME = 10
TIME_SHAPES = ("C4t1", "C4", "C1t")
TIME_PLANS = {("C4", 8): (3, NIT_TIME), ("C4", 9): (3, NIT_TIME), ("C4", 17): (48, 100), ("C4", 25): (44, 40), ("C4t1", 7): (2, NIT_TIME),
              ("C4t1", 9): (9, NIT_TIME), ("C4t1", 25): (2, NIT_TIME)}   # (batch seed, iterations); every other (shape, T): (1, NIT_TIME)
ILL_FACTOR = 10.0
SYSTEM = {"C2": (0, 1), "C2r": (0, 1), "C3": (0, 1), "C2nd": (0, 2), "C4t1": (1, 1), "C4": (1, 2), "C1j": (2, 1), "C1t": (3, 1), "C2h": (0, 1),
          "C2hl": (0, 1), "chain3": (0, 1), "shared": (0, 1), "limits": (0, 1)}


def make_case(ctx, name, T, kp=None):
    """(cfg, desc, inp, systems): workload `name` at horizon T on B instances and the oracle's System of every instance."""
    if name == "chain3":
        cfg = dict(nc.narrow_cfg("C2", 3), T=T)
        desc, inp = workloads.make_batch(ctx, cfg, B=B, chain=nc.capi_chain(3))
        segs = nc.oracle_segs(3)
        return cfg, desc, inp, [nc.oracle_system(cfg, inp, i, segs) for i in range(B)]
    if name == "shared":  # the final keypoint plus one with the same target and another precision, against one keypoint with the summed precision
        cfg, desc, inp, cfg_eq, inp_eq = ss.make_case(ctx, "C2", "sum", B, T=T)
        return cfg, desc, inp, [oracle_system_of_instance(cfg_eq, inp_eq, i) for i in range(B)]
    if name == "limits":  # the chain's own joint limits: the perturbed executions cross them
        cfg = dict(workloads.config("C2"), T=T)
        desc, inp = workloads.make_batch(ctx, cfg, B=B, limits="chain")
    elif name in TIME_SHAPES:  # tests/horizons.make_case with the batch seed of TIME_SEEDS
        cfg = dict(workloads.config(name), T=T, shape=name)
        desc, inp = workloads.make_batch(ctx, cfg, B=B, seed=TIME_PLANS.get((name, T), (1, NIT_TIME))[0], kp_t=kp)
        inp["U0"][:, :, -1] = np.sqrt(cfg["ctimes"][-1] / (T - 1))
    else:
        cfg, desc, inp = hz.make_case(ctx, name, T, B=B, kp=kp)
    return cfg, desc, inp, [oracle_system_of_instance(cfg, inp, i) for i in range(B)]


def solve(ctx, cfg, desc, inp):
    p = workloads.load_batch(ctx, desc, inp, len(inp["q0"]))
    nit = TIME_PLANS.get((cfg.get("shape"), cfg["T"]), (1, NIT_TIME))[1] if cfg.get("ctimes") else NIT
    workloads.run_solver(p, cfg, nb_iter=nit, early_stop=True)
    return p


def plan_of(p):
    """The plan as the getters return it (d is alpha d_k already: ilqr_problem_get_d)."""
    return dict(X=p.X(), U=p.U(), K=p.K(), d=p.d(), cost=p.cost())


def perturbations(plan, S, seed):
    """x0 = xbar_0 + 1e-2 N(0, 1) as in the tracking test, w = 1e-3 N(0, 1)."""
    rng = np.random.default_rng(seed)
    Bn, T, nx = plan["X"].shape
    x0 = plan["X"][:, None, 0, :] + 1e-2 * rng.standard_normal((Bn, S, nx))
    w = 1e-3 * rng.standard_normal((Bn, S, T - 1, nx))
    return x0, w


def replay_one(s, plan, b, x0, w, ff, wide=False):
    """The law for one sample of instance b: (X [T][n_x], U [T-1][n_u], J).  wide: the gain product accumulated in np.longdouble."""
    Xb, Ub, K, d = plan["X"][b], plan["U"][b], plan["K"][b], plan["d"][b]
    T = Xb.shape[0]
    X, U = np.zeros((T, Xb.shape[1])), np.zeros((T - 1, Ub.shape[1]))
    x, J = np.array(x0, dtype=np.float64), 0.0
    for k in range(T - 1):
        X[k] = x
        if wide:
            ld = np.longdouble
            u = Ub[k].astype(ld) + K[k].astype(ld) @ (x.astype(ld) - Xb[k].astype(ld))
            u = np.asarray((u + d[k].astype(ld)) if ff else u, dtype=np.float64)
        else:
            u = Ub[k] + K[k] @ (x - Xb[k])
            if ff:
                u = u + d[k]
        U[k] = u
        J += orc.cost(s, x, u, k)
        x = orc.step(s, x, u)[0]
        if w is not None:
            x = x + w[k]
    X[T - 1] = x
    J += orc.cost(s, x, np.zeros(Ub.shape[1]), T - 1)
    return X, U, J


def _within(got, ref):
    """per step: |got - ref| <= 1e-9 max(1, |ref_k|_inf)"""
    tol = 1e-9 * np.maximum(1.0, np.abs(ref).max(axis=-1, keepdims=True))
    return bool(np.all(np.abs(got - ref) <= tol))


def check_against_replay(systems, plan, x0, w, ff, cost, X, U, tag, stats):
    """(a) and (b) for every sample; stats: dict(n, ill, worst_ratio, worst_X, worst_U, worst_J) updated in place."""
    Bn, S = cost.shape
    for b in range(Bn):
        for s in range(S):
            x0s = x0[b, s] if x0 is not None else plan["X"][b, 0]
            ws = w[b, s] if w is not None else None
            Xr, Ur, Jr = replay_one(systems[b], plan, b, x0s, ws, ff)
            assert np.all(np.isfinite(Xr)) and np.all(np.isfinite(Ur)) and np.isfinite(Jr), f"{tag}: the replay of sample ({b}, {s}) is not finite"
            dX, dU = float(np.abs(X[b, s] - Xr).max()), float(np.abs(U[b, s] - Ur).max())
            dJ = abs(cost[b, s] - Jr) / max(abs(Jr), 1e-300)
            stats["n"] += 1
            ok = _within(X[b, s], Xr) and _within(U[b, s], Ur) and dJ <= 1e-9
            if not ok:  # ill-conditioned: what the replay itself moves under a wider accumulation of its gain product
                Xw, Uw, Jw = replay_one(systems[b], plan, b, x0s, ws, ff, wide=True)
                sX, sU, sJ = float(np.abs(Xw - Xr).max()), float(np.abs(Uw - Ur).max()), abs(Jw - Jr) / max(abs(Jr), 1e-300)
                ratio = 0.0
                for name, dev, sens, fine in (("X", dX, sX, _within(X[b, s], Xr)), ("U", dU, sU, _within(U[b, s], Ur)), ("J", dJ, sJ, dJ <= 1e-9)):
                    if fine:
                        continue
                    assert dev <= ILL_FACTOR * sens, (f"{tag}: {name} of sample ({b}, {s}) is {dev:.3e} from the replay, which its own wider "
                                                      f"accumulation moves by {sens:.3e}")
                    ratio = max(ratio, dev / sens)
                stats["ill"] += 1
                stats["worst_ratio"] = max(stats["worst_ratio"], ratio)
            else:
                stats["worst_X"], stats["worst_U"], stats["worst_J"] = max(stats["worst_X"], dX), max(stats["worst_U"], dU), max(stats["worst_J"], dJ)


def new_stats():
    return dict(n=0, ill=0, worst_ratio=0.0, worst_X=0.0, worst_U=0.0, worst_J=0.0)


def check_definition(p, X, U, ff, tag):
    """(c): every control is what ilqr_problem_track returns for the state it was computed from."""
    S, T = X.shape[1], X.shape[2]
    for s in range(S):
        for k in range(T - 1):
            ut = p.track(k, X[:, s, k], ff)
            assert _within(U[:, s, k], ut), f"{tag}: U[:, {s}, {k}] is not track({k}, X[:, {s}, {k}], {ff}): {np.abs(U[:, s, k] - ut).max():.3e}"


def check_null(p, cfg, plan, S, tag):
    """(d)"""
    cost, X, U = p.closed_loop(samples=S)
    assert cost.shape == (plan["X"].shape[0], S)
    for s in range(S):
        assert _within(X[:, s], plan["X"]), f"{tag}: the undisturbed closed loop leaves the plan by {np.abs(X[:, s] - plan['X']).max():.3e}"
        assert _within(U[:, s], plan["U"]), tag
        if cfg["solver"] == "recursive":
            np.testing.assert_allclose(cost[:, s], plan["cost"], rtol=1e-9, atol=0, err_msg=tag)
        assert np.array_equal(cost[:, s], cost[:, 0]) and np.array_equal(X[:, s], X[:, 0]) and np.array_equal(U[:, s], U[:, 0]), f"{tag}: copies differ"


@contextlib.contextmanager
def generic_pin():
    """The generic kernels for the calls inside (capi.BatchProblem applies ILQR_HIP_PATH at every call)."""
    old = os.environ.get("ILQR_HIP_PATH")
    os.environ["ILQR_HIP_PATH"] = "v1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["ILQR_HIP_PATH"]
        else:
            os.environ["ILQR_HIP_PATH"] = old


def check_case(ctx, name, T, samples, kp=None, definition=True, stats=None, compare_generic=False):
    """One plan, every S of `samples`: (a), (b) for both ff, (c), (d); compare_generic: (e), the same calls under the generic pin return the
    same bits.  Returns a one-line summary."""
    cfg, desc, inp, systems = make_case(ctx, name, T, kp=kp)
    stats = stats if stats is not None else new_stats()
    n0, ill0 = stats["n"], stats["ill"]
    p = solve(ctx, cfg, desc, inp)
    try:
        plan = plan_of(p)
        nlim = 0
        for S in samples:
            tag = f"{name} T={T} S={S}"
            x0, w = perturbations(plan, S, seed=1000 * T + S)
            for ff in (False, True):
                cost, X, U = p.closed_loop(x0, w, with_feedforward=ff)
                assert np.all(np.isfinite(cost)) and np.all(np.isfinite(X)) and np.all(np.isfinite(U)), f"{tag}: non-finite result"
                check_against_replay(systems, plan, x0, w, ff, cost, X, U, f"{tag} ff={ff}", stats)
                if definition:
                    check_definition(p, X, U, ff, f"{tag} ff={ff}")
                if compare_generic:
                    with generic_pin():
                        cg, Xg, Ug = p.closed_loop(x0, w, with_feedforward=ff)
                    assert np.array_equal(cg, cost) and np.array_equal(Xg, X) and np.array_equal(Ug, U), (
                        f"{tag} ff={ff}: the generic kernel differs from the chosen one: cost {np.abs(cg - cost).max():.3e}, X {np.abs(Xg - X).max():.3e}, "
                        f"U {np.abs(Ug - U).max():.3e}")
            c2, X2, U2 = p.closed_loop(x0, w, want_X=False, want_U=False)  # the outputs are optional
            assert X2 is None and U2 is None
            cf, _, _ = p.closed_loop(x0, w)
            assert np.array_equal(c2, cf), f"{tag}: the cost depends on which outputs are asked for"
            if name == "limits":  # the case is about limit terms: some sample must leave the limits
                lim = inp["limits"]
                nlim += int(np.count_nonzero(np.any((X > lim["state_max"]) | (X < lim["state_min"]), axis=(2, 3))))
            check_null(p, cfg, plan, S, tag)
    finally:
        p.close()
    assert name != "limits" or nlim > 0, f"{name} T={T}: no sample leaves the joint limits"
    return (f"{name} T={T} S={tuple(samples)}: {stats['n'] - n0} samples, {stats['ill'] - ill0} by their sensitivity"
            + (f", {nlim} beyond the limits" if name == "limits" else ""))


def _refused(call, text):
    try:
        call()
    except RuntimeError as e:
        assert text in str(e), f"expected an error about {text!r}, got {e}"
    else:
        raise AssertionError(f"expected an error about {text!r}")


def check_interfaces(ctx, device_call, batch_solver=False):
    """(g): each refusal has its own text; the device-pointer entry point returns what the host one does.
    device_call(p, S, x0, w, ff) -> (cost, X, U) through ilqr_problem_closed_loop_dev; batch_solver: a BatchILQR solve counts as no plan."""
    import ctypes as C

    cfg, desc, inp, _ = make_case(ctx, "C2", 9)
    p = workloads.load_batch(ctx, desc, inp, B)
    try:
        _refused(lambda: p.closed_loop(samples=2), "closed loop needs the gains")        # nothing solved yet
        p.solve_recursive(0, True, False)
        _refused(lambda: p.closed_loop(samples=2), "closed loop needs the gains")        # a rollout leaves no gains
        solve_again = lambda: workloads.run_solver(p, cfg, nb_iter=NIT, early_stop=True)  # noqa: E731
        solve_again()
        plan = plan_of(p)
        x0, w = perturbations(plan, 5, seed=5)
        host = p.closed_loop(x0, w, with_feedforward=True)
        _refused(lambda: p.closed_loop(samples=0), "n_samples must be >= 1")
        _refused(lambda: ctx.check(p.L.ilqr_problem_closed_loop(p.h, 1, None, None, 0, None, None, None)), "cost is a null pointer")
        one = np.zeros(1)
        big = (1 << 31) // (B * 9 * p.dims.n_x) + 1   # the check precedes every allocation and launch
        _refused(lambda: ctx.check(p.L.ilqr_problem_closed_loop(p.h, big, None, None, 0, one.ctypes.data_as(C.POINTER(C.c_double)), None, None)),
                 "32-bit offsets")
        dev = device_call(p, 5, x0, w, True)
        for h, d in zip(host, dev):
            assert np.array_equal(h, d), "the device-pointer entry point differs from the host one"
        dev = device_call(p, 5, None, None, False)   # null inputs through the device entry point
        for h, d in zip(p.closed_loop(samples=5), dev):
            assert np.array_equal(h, d)
        if batch_solver:
            p.solve_batch(1)
            _refused(lambda: p.closed_loop(samples=2), "closed loop needs the gains")
            solve_again()
            assert np.array_equal(p.closed_loop(x0, w, with_feedforward=True)[0], host[0])
        p.set_controls(inp["U0"])
        _refused(lambda: p.closed_loop(samples=2), "closed loop needs the gains")        # an input changed
    finally:
        p.close()


def host_pointer_call(p, S, x0, w, ff):
    """ilqr_problem_closed_loop_dev on arrays of the host: what a device pointer is on the host build of the kernels."""
    T, nx, nu = p.T, p.dims.n_x, p.dims.n_u
    x0 = np.ascontiguousarray(x0) if x0 is not None else None
    w = np.ascontiguousarray(w) if w is not None else None
    cost, X, U = np.zeros((p.B, S)), np.zeros((p.B, S, T, nx)), np.zeros((p.B, S, T - 1, nu))
    p.closed_loop_dev(S, x0.ctypes.data if x0 is not None else None, w.ctypes.data if w is not None else None, ff, cost.ctypes.data, X.ctypes.data,
                      U.ctypes.data)
    p.ctx.synchronize()
    return cost, X, U
