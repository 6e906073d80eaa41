"""The I/O-wave form of k_backward_si_dpp (the four chain waves of the workgroup form and a fifth wave that executes no Riccati arithmetic: it
takes the gain image and the accepted x | u of every step out of rings of RING slots in LDS and stores the image where the chain wave stored
it itself and x, u as whole 128-byte row segments of the workgroup's 16 instances; "produced" / "consumed" words in LDS, no barrier in the
step loop) reproduces the one-wave form bit for bit.

Every case solves one seeded problem twice, under ILQR_SWEEP=siwgio and under ILQR_SWEEP=siwave (the reference), with ILQR_HIP_PATH=v2,
ILQR_FWD=wg and everything else pinned alike, and requires np.array_equal(..., equal_nan=True) on cost, X, U, K, d, iters, status and both
traces, and every solve of the file requires that ILQR_STATUS_SWEEP_IO (a bounded wait given up) is set nowhere.  The shapes are those of tests/test_gpu_sweep_wg.py plus what the
ring adds:
  horizons 3, 5, 6, 8, 9, 18   as there (step group PF = 4), and T - 1 in {RING - 1, RING, RING + 1, 2 RING + 1}: the ring not filled, filled
                               exactly, its first slot reused once, every slot reused twice (with RING = 8 only T = 10 is new: 8 horizons)
  batches 1, 5, 16, 17, 67     ragged wave, ragged workgroup, chain waves without an instance inside a live workgroup (the I/O wave skips them)
  records                      C3 (AL, one row, packed symmetric record), C2r (plain record, no AL), C1j (JointSpace)
  acceptances                  no line search, the URDF's bounds with 10 iterations (accepted alpha < 1, asserted), the same with early stop
  AL update                    C3 with 7 iterations at lag 5
  early stop                   4 and 16 copied stoppers: one chain wave stops whole, then a whole workgroup (its I/O wave has nothing to do)
  keypoints                    steps 3, 4 and T - 1
  batch independence           the same 16 instances inside B = 16 and inside B = 67
  fallback                     C3 with two constraint rows: the pin gives the four-wave form's (ILQR_SWEEP=siwg) bits"""
import numpy as np
import pytest

from ilqr_planner_amd import capi, workloads

pytestmark = pytest.mark.gpu

G = 4     # steps per group of the unrolled loop (PF of k_backward_si_dpp)
RING = 8  # SW_RING of ilqr_kernels_dpp.hip: slots per ring
STATUS_SWEEP_IO = capi.STATUS_SWEEP_IO  # ILQR_STATUS_SWEEP_IO of include/ilqr_hip.h
HORIZONS = tuple(sorted({3, 5, 6, 8, 9, 18} | {n + 1 for n in (RING - 1, RING, RING + 1, 2 * RING + 1)}))
BATCHES = (1, 5, 16, 17, 67)
FIELDS = ("cost", "X", "U", "K", "d", "iters", "status", "cost_trace", "alpha_trace")
P = [1, 1, 1, .1, .1, .1]


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
        return dict(cost=p.cost(), X=p.X(), U=p.U(), K=p.K(), d=p.d(), iters=p.iters(), status=st, cost_trace=ct, alpha_trace=at)
    finally:
        p.close()


def _both(ctx, monkeypatch, tag, cfg, desc, inp, nb_iter, ref="siwave", **kw):
    """The solve under the I/O-wave form and under the reference form, bit-equal in every output; returns the I/O-wave form's."""
    new = _solve(ctx, monkeypatch, "siwgio", cfg, desc, inp, nb_iter, **kw)
    old = _solve(ctx, monkeypatch, ref, cfg, desc, inp, nb_iter, **kw)
    for f in FIELDS:
        if not np.array_equal(new[f], old[f], equal_nan=True):
            bad = np.argwhere(~((new[f] == old[f]) | (np.isnan(new[f]) & np.isnan(old[f]))))
            raise AssertionError(f"{tag}: {f} differs between ILQR_SWEEP=siwgio and {ref} at {len(bad)} entries, first {bad[0].tolist()}: "
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
    """The URDF's joint bounds: the limit cost makes the line search reject full steps, so the sweep stores blended x, u."""
    cfg, desc, inp = _case(ctx, name, 18, 67, limits="urdf")
    out = _both(ctx, monkeypatch, f"{name} limits", cfg, desc, inp, 10)
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
    instances 0 .. n_copy - 1: with 4 one chain wave stops whole (the I/O wave must not wait for it) while other stoppers leave their waves in
    part, with 16 a whole workgroup stops."""
    nb_iter = 14
    cfg, desc, inp = _case(ctx, "C3", 17, 67)
    it0 = _solve(ctx, monkeypatch, "siwgio", cfg, desc, inp, nb_iter, early_stop=True)["iters"]
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
    Q = [P, P, P] if name == "C3" else [[1, 1, 1, 0, 0, 0]] * 3
    cfg, desc, inp = _case(ctx, name, T, 17, kp_t=(G - 1, G, T - 1), Qdiag=Q)
    _both(ctx, monkeypatch, f"{name} T={T} keypoints {G - 1}, {G}, {T - 1}", cfg, desc, inp, 4)


def test_batch_size_independence(ctx, monkeypatch):
    """The first 16 instances of a batch of 67, solved inside it and as a batch of their own: the same bits under ILQR_SWEEP=siwgio."""
    cfg, desc, inp = _case(ctx, "C3", 18, 67)
    n = 16
    sub = {k: (v[:n] if isinstance(v, np.ndarray) and v.shape[:1] == (67,) else v) for k, v in inp.items()}
    sub["targets"] = [t[:n] for t in inp["targets"]]
    big = _solve(ctx, monkeypatch, "siwgio", cfg, desc, inp, 4)
    small = _solve(ctx, monkeypatch, "siwgio", cfg, desc, sub, 4)
    for f in FIELDS:
        assert np.array_equal(big[f][:n], small[f], equal_nan=True), f"{f} of the first {n} instances depends on the batch size"


def test_two_rows_fall_back(ctx, monkeypatch):
    """Two constraint rows (the MR = 4 instantiation, which has no I/O-wave form): the pin runs the four-wave workgroup form, ILQR_SWEEP=siwg's bits."""
    cfg, desc, inp = _case(ctx, "C3", 18, 67)
    B, T = 67, 18
    A = np.zeros((2, inp["A"].shape[1]))
    A[0] = inp["A"][0]
    A[1, (cfg["al"]["row"] + 1) % 7] = 1.0
    inp.update(A=A, b=np.array([cfg["al"]["bound"], cfg["al"]["bound"]]), lambda0=np.full((B, T - 1, 2), cfg["al"]["bound"]))
    _both(ctx, monkeypatch, "C3 with two rows", cfg, desc, inp, 7, ref="siwg")
    _both(ctx, monkeypatch, "C3 with two rows", cfg, desc, inp, 7, ref="siwave")
