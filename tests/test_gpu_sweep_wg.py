"""The workgroup form of k_backward_si_dpp (four waves = 16 consecutive instances per workgroup, so that the waves which share every 128-byte line
of x, u run on one CU; a wave's first instance is (tile * 4 + wave) * 4, its gain image its own part of the workgroup's LDS) reproduces the
one-wave form bit for bit.

Every case solves one seeded problem twice, under ILQR_SWEEP=siwg and under ILQR_SWEEP=siwave (the reference), with ILQR_HIP_PATH=v2, ILQR_FWD=wg
and everything else pinned alike, and requires np.array_equal(..., equal_nan=True) on cost, X, U, K, d, iters, status and both traces (K and d: the
gain path shares the kernel).  The shapes are the smallest at which the form can go wrong (prefetch ring / step group PF = G = 4):
  horizons 3, 5, 6, 8, 9, 18   shorter than one group, (T - 1) mod 4 in {0, 1, 3}, (T - 2) mod 4 = 3 (T = 5, 9: the tail sends the last gain image itself)
  batches 1, 5, 16, 17, 67     ragged wave (4 instances), ragged workgroup (16), waves without an instance inside a live workgroup
  records                      C3 (AL, uniform R: packed symmetric), C2r (plain, no AL), C1j (JointSpace)
  acceptances                  no line search (every winner alpha = 1: nothing may be stored), the URDF's bounds with 10 iterations (accepted
                               alpha < 1: the accepted x, u are stored over x(1), u(1)), the same with early stop (stopped instances beside blending ones)
  AL update                    C3 with 7 iterations: a sweep after a multiplier update (lag 5)
  early stop                   one wave stops whole while others stop in part; a whole workgroup of 16 instances stops
  keypoints                    steps 3, 4 and T - 1: both sides of a group boundary and the terminal step
and the same 16 instances give the same bits inside B = 16 and inside B = 67."""
import numpy as np
import pytest

from ilqr_planner_amd import workloads

pytestmark = pytest.mark.gpu

G = 4  # steps per group of the unrolled loop (PF of k_backward_si_dpp)
HORIZONS = (3, 5, 6, 8, 9, 18)
BATCHES = (1, 5, 16, 17, 67)
FIELDS = ("cost", "X", "U", "K", "d", "iters", "status", "cost_trace", "alpha_trace")
P = [1, 1, 1, .1, .1, .1]


@pytest.fixture(scope="module")
def ctx():
    from ilqr_planner_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


def _solve(ctx, monkeypatch, sweep, cfg, desc, inp, nb_iter, early_stop=False, line_search=True):
    for k in ("ILQR_APPLY", "ILQR_CP", "ILQR_CP_SOLVE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ILQR_HIP_PATH", "v2")
    monkeypatch.setenv("ILQR_FWD", "wg")
    monkeypatch.setenv("ILQR_SWEEP", sweep)
    p = workloads.load_batch(ctx, desc, inp, len(inp["q0"]))
    try:
        if cfg["solver"] == "al":
            al = cfg["al"]
            p.solve_al(nb_iter, al["lag"], al["penalty"], al["scaling"], line_search, early_stop)
        else:
            p.solve_recursive(nb_iter, line_search, early_stop)
        ct, at = p.trace(nb_iter)
        return dict(cost=p.cost(), X=p.X(), U=p.U(), K=p.K(), d=p.d(), iters=p.iters(), status=p.status(), cost_trace=ct, alpha_trace=at)
    finally:
        p.close()


def _both(ctx, monkeypatch, tag, cfg, desc, inp, nb_iter, **kw):
    """The solve under both forms, bit-equal in every output; returns the workgroup form's."""
    new = _solve(ctx, monkeypatch, "siwg", cfg, desc, inp, nb_iter, **kw)
    old = _solve(ctx, monkeypatch, "siwave", cfg, desc, inp, nb_iter, **kw)
    for f in FIELDS:
        if not np.array_equal(new[f], old[f], equal_nan=True):
            bad = np.argwhere(~((new[f] == old[f]) | (np.isnan(new[f]) & np.isnan(old[f]))))
            raise AssertionError(f"{tag}: {f} differs between ILQR_SWEEP=siwg and siwave at {len(bad)} entries, first {bad[0].tolist()}: "
                                 f"{new[f][tuple(bad[0])]!r} against {old[f][tuple(bad[0])]!r}")
    assert new["iters"].max() > 0, f"{tag}: no iteration ran"
    return new


def _case(ctx, name, T, B, limits="inactive", kp_t=None, **over):
    cfg = dict(workloads.config(name), T=T, **over)
    desc, inp = workloads.make_batch(ctx, cfg, B=B, limits=limits, kp_t=kp_t)
    return cfg, desc, inp


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
def test_no_line_search(ctx, monkeypatch, name):
    """Every winner is alpha = 1: no instance blends, nothing is stored and the other buffer must stay as the forward pass wrote it."""
    cfg, desc, inp = _case(ctx, name, 18, 67)
    out = _both(ctx, monkeypatch, f"{name} no line search", cfg, desc, inp, 6, line_search=False)
    at = out["alpha_trace"]
    assert np.all(at[np.isfinite(at)] == 1.0), "a step size other than 1 without a line search"


@pytest.mark.parametrize("name", ("C3", "C2r"))
def test_limit_acceptances(ctx, monkeypatch, name):
    """The URDF's joint bounds: the limit cost makes the line search reject full steps, so the sweep stores blended x, u -- beside the waves of
    the ragged last workgroup (3 instances of 16) that hold no instance, and beside alpha = 1 winners where the workload has them (printed)."""
    cfg, desc, inp = _case(ctx, name, 18, 67, limits="urdf")
    nb_iter = 10
    out = _both(ctx, monkeypatch, f"{name} limits", cfg, desc, inp, nb_iter)
    at = out["alpha_trace"]
    print(f"{name} limits: {int(np.sum(at < 1))} of {int(np.sum(np.isfinite(at)))} accepted step sizes below 1, {int(np.sum(at == 1))} equal to 1")
    assert np.any(at < 1), "the line search never went below 1: no entry was stored"


def test_limits_with_early_stop(ctx, monkeypatch):
    """The URDF's bounds with early stop: instances that have left the iteration (no pending acceptance) share workgroups with blending ones."""
    nb_iter = 14
    cfg, desc, inp = _case(ctx, "C3", 18, 67, limits="urdf")
    out = _both(ctx, monkeypatch, "C3 limits, early stop", cfg, desc, inp, nb_iter, early_stop=True)
    it, at = out["iters"], out["alpha_trace"]
    mixed = 0
    for i in range(0, len(it), 16):  # a sweep of iteration t + 1 applies the acceptance of iteration t: after the first stop of the workgroup, before the last iteration
        wi, wa = it[i:i + 16], at[i:i + 16]
        if (wi < nb_iter).any() and (wa[wi == nb_iter, wi.min():nb_iter - 1] < 1).any():
            mixed += 1
    print(f"limits + early stop: iterations {np.bincount(it).tolist()}, {mixed} workgroups with a stopped instance beside one that blends afterwards")
    assert mixed >= 1, "no workgroup mixes stopped and blending instances"


@pytest.mark.parametrize("T", (6, 18))
def test_al_update(ctx, monkeypatch, T):
    """Seven iterations with lag 5: the sweep of iteration 5 applies a multiplier update."""
    cfg, desc, inp = _case(ctx, "C3", T, 17)
    assert cfg["al"]["lag"] == 5
    _both(ctx, monkeypatch, f"C3 T={T} AL update", cfg, desc, inp, 7)


@pytest.mark.parametrize("n_copy", (4, 16))
def test_early_stop(ctx, monkeypatch, n_copy):
    """Instances that stop early beside instances that run on.  A first solve finds an instance that stops; its inputs are then copied over
    instances 0 .. n_copy - 1: with 4 one wave stops whole while other stoppers leave their waves in part, with 16 a whole workgroup stops."""
    nb_iter = 14
    cfg, desc, inp = _case(ctx, "C3", 17, 67)
    it0 = _solve(ctx, monkeypatch, "siwg", cfg, desc, inp, nb_iter, early_stop=True)["iters"]
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
    groups = sum(bool(stopped[i:i + 16].all()) for i in range(0, len(it), 16))
    print(f"early stop: {int(stopped.sum())} of {len(it)} instances stopped (iterations {np.bincount(it).tolist()}), "
          f"{whole} waves stopped whole, {part} in part, {groups} workgroups whole")
    assert stopped.any() and (~stopped).any(), f"need instances that stop and instances that go on, iterations {np.bincount(it).tolist()}"
    assert whole >= 1 and part >= 1, f"need a wave that stops whole and one that stops in part: {whole} whole, {part} in part"
    if n_copy == 16:
        assert stopped[:16].all(), "the first workgroup did not stop whole"


@pytest.mark.parametrize("T", (9, 18))
@pytest.mark.parametrize("name", ("C3", "C2r"))
def test_three_keypoints(ctx, monkeypatch, name, T):
    Q = [P, P, P] if name == "C3" else [[1, 1, 1, 0, 0, 0]] * 3
    cfg, desc, inp = _case(ctx, name, T, 17, kp_t=(G - 1, G, T - 1), Qdiag=Q)
    _both(ctx, monkeypatch, f"{name} T={T} keypoints {G - 1}, {G}, {T - 1}", cfg, desc, inp, 4)


def test_batch_size_independence(ctx, monkeypatch):
    """The first 16 instances of a batch of 67, solved inside it and as a batch of their own: the same bits under ILQR_SWEEP=siwg."""
    cfg, desc, inp = _case(ctx, "C3", 18, 67)
    n = 16
    sub = {k: (v[:n] if isinstance(v, np.ndarray) and v.shape[:1] == (67,) else v) for k, v in inp.items()}
    sub["targets"] = [t[:n] for t in inp["targets"]]
    big = _solve(ctx, monkeypatch, "siwg", cfg, desc, inp, 4)
    small = _solve(ctx, monkeypatch, "siwg", cfg, desc, sub, 4)
    for f in FIELDS:
        assert np.array_equal(big[f][:n], small[f], equal_nan=True), f"{f} of the first {n} instances depends on the batch size"
