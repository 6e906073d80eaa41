"""k_forward_reg with helper waves (ILQR_FWD=wgio: a gain loader, an x | u loader and a storer per workgroup carry the loop's loads and line
stores, the four chain waves keep the arithmetic and meet the helpers through rings and flag words in LDS) reproduces k_forward_wg bit for bit.

Every case solves one seeded problem twice, under ILQR_FWD=wgio and under ILQR_FWD=wglds (k_forward_wg, the bitwise reference), everything else
pinned alike, and requires np.array_equal(..., equal_nan=True) on cost, X, U, iters, status and both traces; every solve under wgio also requires
that ILQR_STATUS_SWEEP_IO (a bounded wait given up) is set nowhere.  The cases are those of tests/test_gpu_forward_reg.py with the horizons set
against the form's ring of FIO_RING = 8 steps and the chain waves' group of FIO_GROUP = 4 (ilqr_fwd_io_plan.hpp):
  T - 1 in 2, 4, 5, 7, 8, 9, 17   shorter than a group; one group, and one step more; one slot short of the ring, the ring, one over; two wraps plus one
  batches 1, 5, 16, 17, 67         a chain wave without an instance, a ragged workgroup, a workgroup whose last three chain waves are dead (the
                                   helpers must not wait for them)
  records                          C3 (AL, uniform R: packed symmetric), C2r (plain), C1j (JointSpace)
  limits                           the URDF's bounds, with the line search below 1 and a bound exceeded: the limit branch ran
  step sizes                       no line search (one step size), alpha_floor = 4e-5 (sixteen)
  early stop                       a chain wave that stops whole beside waves that stop in part; a whole workgroup (16 instances) that has stopped while
                                   others run on: the workgroup-uniform exit, with which the helpers must end too
  keypoints                        steps 7, 8 and T - 1: both sides of a group boundary and the terminal step
and the same 16 instances give the same bits inside B = 16 and inside B = 67."""
import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads

pytestmark = pytest.mark.gpu

HORIZONS = (3, 5, 6, 8, 9, 10, 18)
BATCHES = (1, 5, 16, 17, 67)
FIELDS = ("cost", "X", "U", "iters", "status", "cost_trace", "alpha_trace")
P = [1, 1, 1, .1, .1, .1]
STATUS_SWEEP_IO = capi.STATUS_SWEEP_IO  # ILQR_STATUS_SWEEP_IO of include/ilqr_hip.h


@pytest.fixture(scope="module")
def ctx():
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
        st = p.status()
        assert not np.any(st & STATUS_SWEEP_IO), f"ILQR_FWD={fwd}: a wave gave up a bounded wait (ILQR_STATUS_SWEEP_IO) at instances {np.flatnonzero(st & STATUS_SWEEP_IO).tolist()}"
        return dict(cost=p.cost(), X=p.X(), U=p.U(), iters=p.iters(), status=st, cost_trace=ct, alpha_trace=at)
    finally:
        p.close()


def _both(ctx, monkeypatch, tag, cfg, desc, inp, nb_iter, **kw):
    """The solve under both kernels, bit-equal in every output; returns the new form's."""
    new = _solve(ctx, monkeypatch, "wgio", cfg, desc, inp, nb_iter, **kw)
    old = _solve(ctx, monkeypatch, "wglds", cfg, desc, inp, nb_iter, **kw)
    for f in FIELDS:
        if not np.array_equal(new[f], old[f], equal_nan=True):
            bad = np.argwhere(~((new[f] == old[f]) | (np.isnan(new[f]) & np.isnan(old[f]))))
            raise AssertionError(f"{tag}: {f} differs between ILQR_FWD=wgio and wglds at {len(bad)} entries, first {bad[0].tolist()}: "
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
    cfg, desc, inp = _case(ctx, "C3", 18, 17, limits=limits)
    if steps == 16:
        desc.alpha_floor = 4e-5
    _both(ctx, monkeypatch, f"C3 {steps} step size(s), limits {limits}", cfg, desc, inp, 6, line_search=steps > 1)


@pytest.mark.parametrize("n_copy", (4, 16))
def test_early_stop(ctx, monkeypatch, n_copy):
    """Instances that stop early beside instances that run on.  A first solve finds an instance that stops; its inputs are then copied over
    instances 0 .. n_copy - 1: with 4, one chain wave stops whole (the helpers of its workgroup no longer wait for it) while the other stoppers
    leave their waves in part; with 16, a whole workgroup has stopped while others run on, and its seven waves leave by the uniform exit."""
    nb_iter = 14
    cfg, desc, inp = _case(ctx, "C3", 18, 67)
    it0 = _solve(ctx, monkeypatch, "wgio", cfg, desc, inp, nb_iter, early_stop=True)["iters"]
    assert (it0 < nb_iter).any(), f"no instance stops early, iterations {np.bincount(it0).tolist()}"
    s = int(np.argmax(it0 < nb_iter))
    for k in ("q0", "dq0", "U0", "lambda0"):
        inp[k][:n_copy] = inp[k][s]
    for t in inp["targets"]:
        t[:n_copy] = t[s]
    out = _both(ctx, monkeypatch, f"C3 early stop, {n_copy} copies", cfg, desc, inp, nb_iter, early_stop=True)
    it = out["iters"]
    stopped = it < nb_iter
    waves = [stopped[i:i + 4] for i in range(0, len(it), 4)]
    whole, part = sum(bool(w.all()) for w in waves), sum(bool(w.any() and not w.all()) for w in waves)
    print(f"early stop: {int(stopped.sum())} of {len(it)} instances stopped (iterations {np.bincount(it).tolist()}), "
          f"{whole} waves stopped whole, {part} in part")
    assert stopped.any() and (~stopped).any(), f"need instances that stop and instances that go on, iterations {np.bincount(it).tolist()}"
    assert stopped[:n_copy].all(), "the copies of a stopping instance did not stop"
    if n_copy == 4:
        assert whole >= 1 and part >= 1, f"need a wave that stops whole and one that stops in part: {whole} whole, {part} in part"
    else:
        assert (~stopped[16:]).any() and it[:16].max() < it[16:].max(), "need a workgroup that has stopped while another runs on"


@pytest.mark.parametrize("T", (18, 26))
@pytest.mark.parametrize("name", ("C3", "C2r"))
def test_three_keypoints(ctx, monkeypatch, name, T):
    Q = [P, P, P] if name == "C3" else [[1, 1, 1, 0, 0, 0]] * 3
    cfg, desc, inp = _case(ctx, name, T, 17, kp_t=(7, 8, T - 1), Qdiag=Q)
    _both(ctx, monkeypatch, f"{name} T={T} keypoints 7, 8, {T - 1}", cfg, desc, inp, 4)


def test_batch_size_independence(ctx, monkeypatch):
    """The first 16 instances of a batch of 67, solved inside it and as a batch of their own: the same bits under ILQR_FWD=wgio."""
    cfg, desc, inp = _case(ctx, "C3", 18, 67)
    n = 16
    sub = {k: (v[:n] if isinstance(v, np.ndarray) and v.shape[:1] == (67,) else v) for k, v in inp.items()}
    sub["targets"] = [t[:n] for t in inp["targets"]]
    big = _solve(ctx, monkeypatch, "wgio", cfg, desc, inp, 4)
    small = _solve(ctx, monkeypatch, "wgio", cfg, desc, sub, 4)
    for f in FIELDS:
        assert np.array_equal(big[f][:n], small[f], equal_nan=True), f"{f} of the first {n} instances depends on the batch size"
