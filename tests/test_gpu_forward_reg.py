"""k_forward_reg, the large-batch forward pass of the single-integrator systems (16 lanes per instance on registers, gain records through a
wave-local LDS ring), reproduces its predecessor k_forward_wg bit for bit.

Every case solves one seeded problem twice, under ILQR_FWD=wg (k_forward_reg at any batch size) and under ILQR_FWD=wglds (k_forward_wg, kept
as the reference), everything else pinned alike, and requires np.array_equal(..., equal_nan=True) on cost, X, U, iters, status and both
traces.  The shapes are the smallest at which the new kernel takes another path:
  horizons 3, 9, 10, 17, 26   shorter than the prefetch ring (8 steps), (T - 1) mod 8 in {0, 1, 7}, a terminal step right behind a ring wrap
  batches 1, 5, 16, 17, 67     ragged wave (4 instances), ragged workgroup (16), a wave without an instance
  records                      C3 (AL, uniform R: packed symmetric), C2r (plain), C1j (JointSpace)
  limits                       the URDF's bounds, with the line search below 1 and a bound exceeded: the limit branch ran
  step sizes                   no line search (one step size), alpha_floor = 4e-5 (sixteen)
  early stop                   instances that stop beside instances that go on: partial and whole-wave `active` masks
  keypoints                    steps 7, 8 and T - 1: both sides of an 8-step group and the terminal step
and the same 16 instances give the same bits inside B = 16 and inside B = 67."""
import numpy as np
import pytest

from ilqr_planner_amd import workloads

pytestmark = pytest.mark.gpu

HORIZONS = (3, 9, 10, 17, 26)
BATCHES = (1, 5, 16, 17, 67)
FIELDS = ("cost", "X", "U", "iters", "status", "cost_trace", "alpha_trace")
P = [1, 1, 1, .1, .1, .1]


@pytest.fixture(scope="module")
def ctx():
    from ilqr_planner_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


def _solve(ctx, monkeypatch, fwd, cfg, desc, inp, nb_iter, early_stop=False, line_search=True):
    for k in ("ILQR_SWEEP", "ILQR_APPLY", "ILQR_CP", "ILQR_CP_SOLVE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ILQR_HIP_PATH", "v2")
    monkeypatch.setenv("ILQR_FWD", fwd)
    p = workloads.load_batch(ctx, desc, inp, len(inp["q0"]))
    try:
        if cfg["solver"] == "al":
            al = cfg["al"]
            p.solve_al(nb_iter, al["lag"], al["penalty"], al["scaling"], line_search, early_stop)
        else:
            p.solve_recursive(nb_iter, line_search, early_stop)
        ct, at = p.trace(nb_iter)
        return dict(cost=p.cost(), X=p.X(), U=p.U(), iters=p.iters(), status=p.status(), cost_trace=ct, alpha_trace=at)
    finally:
        p.close()


def _both(ctx, monkeypatch, tag, cfg, desc, inp, nb_iter, **kw):
    """The solve under both kernels, bit-equal in every output; returns the new kernel's."""
    new = _solve(ctx, monkeypatch, "wg", cfg, desc, inp, nb_iter, **kw)
    old = _solve(ctx, monkeypatch, "wglds", cfg, desc, inp, nb_iter, **kw)
    for f in FIELDS:
        if not np.array_equal(new[f], old[f], equal_nan=True):
            bad = np.argwhere(~((new[f] == old[f]) | (np.isnan(new[f]) & np.isnan(old[f]))))
            raise AssertionError(f"{tag}: {f} differs between ILQR_FWD=wg and wglds at {len(bad)} entries, first {bad[0].tolist()}: "
                                 f"{new[f][tuple(bad[0])]!r} against {old[f][tuple(bad[0])]!r}")
    assert new["iters"].max() > 0, f"{tag}: no iteration ran"
    return new


def _case(ctx, name, T, B, limits="inactive", kp_t=None, **over):
    cfg = dict(workloads.config(name), T=T, **over)
    desc, inp = workloads.make_batch(ctx, cfg, B=B, limits=limits, kp_t=kp_t)
    return cfg, desc, inp


def _limit_cost(inp, X):
    """Limit cost of the accepted trajectories, per instance (penalty 1): sum of squared distances beyond the bounds."""
    lim = inp["limits"]
    w = lim["limit_weight"] != 0
    over = np.maximum(X[:, :, :len(w)] - lim["state_max"], 0.0) + np.maximum(lim["state_min"] - X[:, :, :len(w)], 0.0)
    return (over[:, :, w] ** 2).sum(axis=(1, 2))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("T", HORIZONS)
@pytest.mark.parametrize("name", ("C3", "C2r"))
def test_horizons_and_batches(ctx, monkeypatch, name, T, B):
    cfg, desc, inp = _case(ctx, name, T, B)
    _both(ctx, monkeypatch, f"{name} T={T} B={B}", cfg, desc, inp, 4)


@pytest.mark.parametrize("T", HORIZONS)
def test_joint_space(ctx, monkeypatch, T):
    cfg, desc, inp = _case(ctx, "C1j", T, 17)
    _both(ctx, monkeypatch, f"C1j T={T}", cfg, desc, inp, 4)


@pytest.mark.parametrize("name", ("C3", "C2r"))
def test_limits(ctx, monkeypatch, name):
    """The URDF's joint bounds: targets drawn over the whole joint range pull some joints past them, the limit cost makes the line search
    reject full steps."""
    cfg, desc, inp = _case(ctx, name, 26, 67, limits="urdf")
    nb_iter = 10
    out = _both(ctx, monkeypatch, f"{name} limits", cfg, desc, inp, nb_iter)
    at, lc = out["alpha_trace"], _limit_cost(inp, out["X"])
    print(f"{name} limits: {int(np.sum(at < 1))} of {int(np.sum(np.isfinite(at)))} accepted step sizes below 1, limit cost > 0 in {int(np.sum(lc > 0))} of {len(lc)} instances")
    assert np.any(at < 1), "the line search never went below 1"
    assert np.any(lc > 0), "no instance ends beyond a bound: the limit branch may not have run"


@pytest.mark.parametrize("limits", ("inactive", "urdf"))
@pytest.mark.parametrize("steps", (1, 16))
def test_step_sizes(ctx, monkeypatch, steps, limits):
    """One step size (no line search) and sixteen (alpha_floor = 4e-5: 2^-15 is the first at or below it)."""
    cfg, desc, inp = _case(ctx, "C3", 17, 17, limits=limits)
    if steps == 16:
        desc.alpha_floor = 4e-5
    _both(ctx, monkeypatch, f"C3 {steps} step size(s), limits {limits}", cfg, desc, inp, 6, line_search=steps > 1)


def test_early_stop(ctx, monkeypatch):
    """Instances that stop early beside instances that run on: the stopped ones are masked out of their waves by `active`.  A first solve finds
    an instance that stops; its inputs are then copied over instances 0 .. 3, so that one wave (four consecutive instances) stops whole while
    the other stoppers leave their waves in part."""
    nb_iter = 14
    cfg, desc, inp = _case(ctx, "C3", 17, 67)
    it0 = _solve(ctx, monkeypatch, "wg", cfg, desc, inp, nb_iter, early_stop=True)["iters"]
    assert (it0 < nb_iter).any(), f"no instance stops early, iterations {np.bincount(it0).tolist()}"
    s = int(np.argmax(it0 < nb_iter))
    for k in ("q0", "dq0", "U0", "lambda0"):
        inp[k][:4] = inp[k][s]
    for t in inp["targets"]:
        t[:4] = t[s]
    out = _both(ctx, monkeypatch, "C3 early stop", cfg, desc, inp, nb_iter, early_stop=True)
    it = out["iters"]
    stopped = it < nb_iter
    waves = [stopped[i:i + 4] for i in range(0, len(it), 4)]
    whole, part = sum(bool(w.all()) for w in waves), sum(bool(w.any() and not w.all()) for w in waves)
    print(f"early stop: {int(stopped.sum())} of {len(it)} instances stopped (iterations {np.bincount(it).tolist()}), "
          f"{whole} waves stopped whole, {part} in part")
    assert stopped.any() and (~stopped).any(), f"need instances that stop and instances that go on, iterations {np.bincount(it).tolist()}"
    assert whole >= 1 and part >= 1, f"need a wave that stops whole and one that stops in part: {whole} whole, {part} in part"


@pytest.mark.parametrize("T", (17, 26))
@pytest.mark.parametrize("name", ("C3", "C2r"))
def test_three_keypoints(ctx, monkeypatch, name, T):
    Q = [P, P, P] if name == "C3" else [[1, 1, 1, 0, 0, 0]] * 3
    cfg, desc, inp = _case(ctx, name, T, 17, kp_t=(7, 8, T - 1), Qdiag=Q)
    _both(ctx, monkeypatch, f"{name} T={T} keypoints 7, 8, {T - 1}", cfg, desc, inp, 4)


def test_batch_size_independence(ctx, monkeypatch):
    """The first 16 instances of a batch of 67, solved inside it and as a batch of their own: the same bits under ILQR_FWD=wg."""
    cfg, desc, inp = _case(ctx, "C3", 17, 67)
    n = 16
    sub = {k: (v[:n] if isinstance(v, np.ndarray) and v.shape[:1] == (67,) else v) for k, v in inp.items()}
    sub["targets"] = [t[:n] for t in inp["targets"]]
    big = _solve(ctx, monkeypatch, "wg", cfg, desc, inp, 4)
    small = _solve(ctx, monkeypatch, "wg", cfg, desc, sub, 4)
    for f in FIELDS:
        assert np.array_equal(big[f][:n], small[f], equal_nan=True), f"{f} of the first {n} instances depends on the batch size"
