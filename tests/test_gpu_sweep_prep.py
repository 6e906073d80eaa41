"""The preparing-wave form of k_backward_si_dpp (the four chain waves and the I/O wave of the I/O-wave form plus two preparing waves, which load
xbar, ubar, x(1), u(1) and the multiplier of every step, blend, write x | u into the I/O wave's ring, form the limit terms and the AL bookkeeping
and hand {u, lim, l_x of the limits, I_k, lam + I_k g, beyond} to the chain waves through a ring of RING slots in LDS; "prepared" words in LDS
beside "produced" / "consumed", no barrier in the step loop) reproduces the one-wave form bit for bit.

Every case solves one seeded problem twice, under ILQR_SWEEP=siwgprep and under ILQR_SWEEP=siwave (the reference), with ILQR_HIP_PATH=v2,
ILQR_FWD=wg and everything else pinned alike, and requires np.array_equal(..., equal_nan=True) on cost, X, U, K, d, iters, status, both traces
and the multipliers after the solve, and every solve of the file requires that ILQR_STATUS_SWEEP_IO (a bounded wait given up) is set nowhere.
The shapes are those of tests/test_gpu_sweep_io.py:
  horizons 3, 5, 6, 8, 9, 10, 18  step group PF = 4, and T - 1 in {LEAD - 1, LEAD, LEAD + 1, RING - 1, RING, RING + 1, 2 RING + 1}: a preparing
                               wave writes step n once step n - RING is consumed, so it runs at most LEAD = RING = 8 steps ahead: the lead
                               never reached, reached exactly, the first slot reused, every slot reused twice
  batches 1, 5, 16, 17, 67     ragged wave, ragged workgroup, chain waves (and a preparing wave) without an instance inside a live workgroup
  records                      C3 (AL, one row, packed symmetric record), C2r (plain record, no AL), C1j (JointSpace)
  acceptances                  no line search, the URDF's bounds with 10 iterations (accepted alpha < 1 and a state beyond a bound, both
                               asserted), the same with early stop
  AL update                    C3 with 7 iterations at lag 5: the preparing waves update and store the multipliers
  early stop                   4 and 16 copied stoppers: one chain wave stops whole, then a whole workgroup
  keypoints                    steps 3, 4 and T - 1
  batch independence           the same 16 instances inside B = 16 and inside B = 67
  fallback                     C3 with two constraint rows: the pin gives the four-wave form's (ILQR_SWEEP=siwg) bits
  gains                        BatchProblem.gains() about a batch solver's plan: the bytes of ILQR_SWEEP=siwave"""
import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads

pytestmark = pytest.mark.gpu

G = 4          # steps per group of the unrolled loop (PF of k_backward_si_dpp)
RING = 8       # SW_PRING of ilqr_kernels_dpp.hip: slots of the prepared ring
LEAD = RING    # steps a preparing wave can be ahead of the I/O wave, hence of the chain waves
STATUS_SWEEP_IO = capi.STATUS_SWEEP_IO  # ILQR_STATUS_SWEEP_IO of include/ilqr_hip.h
HORIZONS = tuple(sorted({3, 5, 6, 8, 9, 10, 18} | {n + 1 for n in (LEAD - 1, LEAD, LEAD + 1, RING - 1, RING, RING + 1, 2 * RING + 1)}))
BATCHES = (1, 5, 16, 17, 67)
FIELDS = ("cost", "X", "U", "K", "d", "iters", "status", "cost_trace", "alpha_trace", "lam")
P = [1, 1, 1, .1, .1, .1]
NEW = "siwgprep"


@pytest.fixture(scope="module")
def ctx():
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
        st = p.status()
        assert not np.any(st & STATUS_SWEEP_IO), f"ILQR_SWEEP={sweep}: a wave gave up a bounded wait (ILQR_STATUS_SWEEP_IO) at instances {np.flatnonzero(st & STATUS_SWEEP_IO).tolist()}"
        lam = p.lam() if cfg["solver"] == "al" else np.zeros(0)
        return dict(cost=p.cost(), X=p.X(), U=p.U(), K=p.K(), d=p.d(), iters=p.iters(), status=st, cost_trace=ct, alpha_trace=at, lam=lam)
    finally:
        p.close()


def _both(ctx, monkeypatch, tag, cfg, desc, inp, nb_iter, ref="siwave", **kw):
    """The solve under the preparing-wave form and under the reference form, bit-equal in every output; returns the preparing-wave form's."""
    new = _solve(ctx, monkeypatch, NEW, cfg, desc, inp, nb_iter, **kw)
    old = _solve(ctx, monkeypatch, ref, cfg, desc, inp, nb_iter, **kw)
    for f in FIELDS:
        if not np.array_equal(new[f], old[f], equal_nan=True):
            bad = np.argwhere(~((new[f] == old[f]) | (np.isnan(new[f]) & np.isnan(old[f]))))
            raise AssertionError(f"{tag}: {f} differs between ILQR_SWEEP={NEW} and {ref} at {len(bad)} entries, first {bad[0].tolist()}: "
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


def _beyond_a_bound(X, inp):
    """States of the returned trajectories that lie beyond a weighted bound of inp["limits"]: there the handed-over lim and l_x are non-zero."""
    lim = inp["limits"]
    smax, smin, lw = np.asarray(lim["state_max"], float), np.asarray(lim["state_min"], float), np.asarray(lim["limit_weight"])
    n = len(smax)
    x = X[..., :n]
    return int(np.sum(((x > smax) | (x < smin)) & (lw != 0)))


@pytest.mark.parametrize("name", ("C3", "C2r"))
def test_limit_acceptances(ctx, monkeypatch, name):
    """The URDF's joint bounds: the limit cost makes the line search reject full steps, so the preparing waves blend and the I/O wave stores,
    and states beyond a bound make the handed-over limit terms non-zero."""
    cfg, desc, inp = _case(ctx, name, 18, 67, limits="urdf")
    out = _both(ctx, monkeypatch, f"{name} limits", cfg, desc, inp, 10)
    at = out["alpha_trace"]
    nb = _beyond_a_bound(out["X"], inp)
    print(f"{name} limits: {int(np.sum(at < 1))} of {int(np.sum(np.isfinite(at)))} accepted step sizes below 1, {int(np.sum(at == 1))} equal to 1; "
          f"{nb} states beyond a bound")
    assert np.any(at < 1), "the line search never went below 1: no entry was stored"
    assert nb >= 1, "no state of the returned trajectories lies beyond a bound: lim and the limits' l_x were zero wherever this can tell"


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
    """Seven iterations with lag 5: the sweep of iteration 5 applies a multiplier update, which the preparing waves compute and store."""
    cfg, desc, inp = _case(ctx, "C3", T, 17)
    assert cfg["al"]["lag"] == 5
    out = _both(ctx, monkeypatch, f"C3 T={T} AL update", cfg, desc, inp, 7)
    assert not np.array_equal(out["lam"], inp["lambda0"]), "the multipliers never moved: no update was stored"


@pytest.mark.parametrize("n_copy", (4, 16))
def test_early_stop(ctx, monkeypatch, n_copy):
    """Instances that stop early beside instances that run on.  A first solve finds an instance that stops; its inputs are then copied over
    instances 0 .. n_copy - 1: with 4 one chain wave stops whole (neither the I/O wave nor its preparing wave may wait for it) while other
    stoppers leave their waves in part, with 16 a whole workgroup stops."""
    nb_iter = 14
    cfg, desc, inp = _case(ctx, "C3", 17, 67)
    it0 = _solve(ctx, monkeypatch, NEW, cfg, desc, inp, nb_iter, early_stop=True)["iters"]
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
    assert stopped.any() and (~stopped).any(), f"need instances that stop and instances that go on, iterations {np.bincount(it).tolist()}"
    assert whole >= 1 and part >= 1, f"need a wave that stops whole and one that stops in part: {whole} whole, {part} in part"
    if n_copy == 16:
        assert stopped[:16].all(), "the first workgroup did not stop whole"


@pytest.mark.parametrize("T", (9, 18))
@pytest.mark.parametrize("name", ("C3", "C2r"))
def test_three_keypoints(ctx, monkeypatch, name, T):
    """A keypoint inside a group, at a group's edge and the terminal one: there l_x comes from the keypoint derivatives and only the AL term of the
    preparing wave is added on the chain."""
    Q = [P, P, P] if name == "C3" else [[1, 1, 1, 0, 0, 0]] * 3
    cfg, desc, inp = _case(ctx, name, T, 17, kp_t=(G - 1, G, T - 1), Qdiag=Q)
    _both(ctx, monkeypatch, f"{name} T={T} keypoints {G - 1}, {G}, {T - 1}", cfg, desc, inp, 4)


def test_batch_size_independence(ctx, monkeypatch):
    """The first 16 instances of a batch of 67, solved inside it and as a batch of their own: the same bits under ILQR_SWEEP=siwgprep."""
    cfg, desc, inp = _case(ctx, "C3", 18, 67)
    n = 16
    sub = {k: (v[:n] if isinstance(v, np.ndarray) and v.shape[:1] == (67,) else v) for k, v in inp.items()}
    sub["targets"] = [t[:n] for t in inp["targets"]]
    big = _solve(ctx, monkeypatch, NEW, cfg, desc, inp, 4)
    small = _solve(ctx, monkeypatch, NEW, cfg, desc, sub, 4)
    for f in FIELDS:
        assert np.array_equal(big[f][:n], small[f], equal_nan=True), f"{f} of the first {n} instances depends on the batch size"


def test_two_rows_fall_back(ctx, monkeypatch):
    """Two constraint rows (the MR = 4 instantiation, which has neither an I/O wave nor preparing waves): the pin runs the four-wave workgroup
    form, ILQR_SWEEP=siwg's bits."""
    cfg, desc, inp = _case(ctx, "C3", 18, 67)
    B, T = 67, 18
    A = np.zeros((2, inp["A"].shape[1]))
    A[0] = inp["A"][0]
    A[1, (cfg["al"]["row"] + 1) % 7] = 1.0
    inp.update(A=A, b=np.array([cfg["al"]["bound"], cfg["al"]["bound"]]), lambda0=np.full((B, T - 1, 2), cfg["al"]["bound"]))
    _both(ctx, monkeypatch, "C3 with two rows", cfg, desc, inp, 7, ref="siwg")
    _both(ctx, monkeypatch, "C3 with two rows", cfg, desc, inp, 7, ref="siwave")


def test_gains_about_a_batch_solver_plan(ctx, monkeypatch):
    """ilqr_problem_gains goes through the same dispatch: about the plan a batch solver left, pin 7 gives the bytes of ILQR_SWEEP=siwave."""
    for k in ("ILQR_APPLY", "ILQR_CP", "ILQR_CP_SOLVE", "ILQR_HIP_PATH", "ILQR_FWD"):
        monkeypatch.delenv(k, raising=False)
    for T in (9, 18):
        cfg = dict(workloads.config("C2"), T=T)
        desc, inp = workloads.make_batch(ctx, cfg, B=17)
        p = workloads.load_batch(ctx, desc, inp, 17)
        try:
            monkeypatch.delenv("ILQR_SWEEP", raising=False)
            p.solve_batch(3, True)
            assert np.all(p.iters() >= 1), "the batch solver did not move the plan"
            out = {}
            for pin in (NEW, "siwave"):
                monkeypatch.setenv("ILQR_SWEEP", pin)
                p.gains()
                st = p.status()
                assert not np.any(st & STATUS_SWEEP_IO), f"gains under {pin}: a wave gave up a bounded wait"
                out[pin] = (p.K(), p.d())
            assert np.isfinite(out[NEW][0]).all() and np.any(out[NEW][0] != 0), "no gains"
            assert np.array_equal(out[NEW][0], out["siwave"][0], equal_nan=True), f"T={T}: K of the gains sweep differs between the pins"
            assert np.array_equal(out[NEW][1], out["siwave"][1], equal_nan=True), f"T={T}: d of the gains sweep differs between the pins"
        finally:
            p.close()
