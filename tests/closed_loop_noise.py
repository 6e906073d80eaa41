"""Closed-loop rollouts with device-drawn noise (ilqr_problem_closed_loop_noise) -- a NumPy restatement of the generator's definition in
include/ilqr_hip.h and the checks shared by tests/tools/hostsim/closed_loop_noise_checks.py (host build of the generic kernel) and
tests/test_gpu_closed_loop_noise.py (device kernels).  Cases, plans and the replay come from tests/closed_loop.py.

  (1) the draw is the definition: w_out and X[:, :, 0] - centre against the restatement within 1e-14 sigma max(1, |z|); sigma 0 gives exact 0;
      all sigmas 0 is closed_loop(w = None) bit for bit.  The start draw is read from a call whose centre is 0, where X[:, :, 0] IS the draw
      (added to a centre of size 1 the sum is rounded at 1e-16, above the bound for sigma = 1e-3); with the plan's start as the centre,
      X[:, :, 0] must then be centre + that draw bit for bit.
  (2) the rollout is the existing one: closed_loop(x0 = X[:, :, 0], w = w_out) returns the same bits, both ff.
  (4) cut-outs with instance_offset / sample_offset reproduce the large call bit for bit; another seed changes every sample.
  (5) statistics against NumPy: min, max, n_bad exact, mean 1e-12, variance 1e-10 relative (std / mean >= 1e-3 asserted); finite-only rule.
  (6) the stream is sound: pooled mean, variance and four lag correlations within 4 standard errors, for a fixed seed.
"""
from __future__ import annotations

import numpy as np

from tests import closed_loop as cl

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
STEP_START = 0xFFFFFFFF
MASK = np.uint64(0xFFFFFFFF)
KAT = (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)))
SHAPES = ("C2", "C3", "C2nd", "C4t1", "C4", "C1j", "chain3")   # 7 pairs, n_x = 8, n_x = 15 (last pair half used), mapped n_x = 3
SEED = 12345


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Arrays (broadcast) of 32-bit words held in uint64 -> (r0, r1, r2, r3)."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def normals(seed, instance, sample, k, j):
    """(z0, z1) of the counter (instance, sample, k, j) under `seed`."""
    r0, r1, r2, r3 = philox4x32_10(instance, sample, k, j, seed & 0xFFFFFFFF, seed >> 32)
    u1 = ((((r1 << np.uint64(32)) | r0) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    u2 = ((((r3 << np.uint64(32)) | r2) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)


def draw(seed, Bn, S, steps, nxu, instance_offset=0, sample_offset=0):
    """z[B][S][len(steps)][nxu]: the normals of every entry of the user's state layout at the given steps."""
    b = np.arange(Bn, dtype=np.uint64)[:, None, None, None] + np.uint64(instance_offset)
    s = np.arange(S, dtype=np.uint64)[None, :, None, None] + np.uint64(sample_offset)
    k = np.asarray(steps, dtype=np.uint64)[None, None, :, None]
    j = np.arange((nxu + 1) // 2, dtype=np.uint64)[None, None, None, :]
    z0, z1 = normals(seed, b, s, k, j)
    z = np.empty((Bn, S, len(steps), 2 * ((nxu + 1) // 2)))
    z[..., 0::2], z[..., 1::2] = z0, z1
    return z[..., :nxu]


def sigma_vectors(nxu, scale_w, scale_x0):
    """Every entry drawn but entry 1 of w (a half-used pair) and, from n_x = 6, the pair (4, 5) of w (a pair that is not generated);
    the start draw leaves out entry 0."""
    sw = scale_w * (1.0 - 0.03125 * np.arange(nxu))   # the scale is the largest sigma
    sx = scale_x0 * (1.0 - 0.046875 * np.arange(nxu))
    if nxu > 1:
        sw[1] = 0.0
    if nxu >= 6:
        sw[4:6] = 0.0
    sx[0] = 0.0
    return sw, sx


def scales(name):
    """sigma_w, sigma_x0 scales: the figures of tests/closed_loop.perturbations; the time systems leave their plan's neighbourhood above 1e-3."""
    return (1e-3, 1e-3) if name in cl.TIME_SHAPES else (3e-2, 3e-1)


def _draw_bound(sig, z):
    return 1e-14 * sig * np.maximum(1.0, np.abs(z))


def check_draw(p, plan, S, seed, sw, sx, tag, worst):
    """(1) and (2).  Returns the noise call's result (feed-forward off) for further checks.  worst: dict(dev=...) of the worst |draw - restatement| in
    units of sigma max(1, |z|)."""
    Bn, T, nxu = plan["X"].shape
    zw = draw(seed, Bn, S, range(T - 1), nxu)
    z0 = draw(seed, Bn, S, [STEP_START], nxu)[:, :, 0]
    res = {}
    for ff in (False, True):
        r = p.closed_loop_noise(S, seed, sw, sx, with_feedforward=ff, want_X=True, want_U=True, want_w=True)
        assert np.all(np.isfinite(r.cost)) and np.all(np.isfinite(r.X)) and np.all(np.isfinite(r.U)), f"{tag} ff={ff}: non-finite execution"
        dev = np.abs(r.w - sw * zw)
        assert np.all(dev <= _draw_bound(sw, zw)), f"{tag}: w_out is not the definition: {np.max(dev / np.maximum(_draw_bound(sw, zw), 1e-300)):.3g} bounds"
        assert np.all(r.w[..., sw == 0.0] == 0.0) and not np.any(np.signbit(r.w[..., sw == 0.0])), f"{tag}: sigma 0 must store exact 0"
        with np.errstate(invalid="ignore", divide="ignore"):
            worst["dev"] = max(worst["dev"], float(np.nanmax(np.where(sw > 0, dev / (sw * np.maximum(1.0, np.abs(zw))), 0.0))))
        # (2) the stored start states and disturbances through the existing entry point
        c2, X2, U2 = p.closed_loop(r.X[:, :, 0], r.w, with_feedforward=ff)
        assert np.array_equal(c2, r.cost) and np.array_equal(X2, r.X) and np.array_equal(U2, r.U), (
            f"{tag} ff={ff}: closed_loop(X[:, :, 0], w_out) differs: cost {np.abs(c2 - r.cost).max():.3e}, X {np.abs(X2 - r.X).max():.3e}")
        res[ff] = r
    # the start draw, read where the centre is 0 (only X[:, :, 0] of that call means anything)
    zero = p.closed_loop_noise(S, seed, None, sx, x0=np.zeros((Bn, S, nxu)), want_cost=True, want_stats=False, want_X=True)
    d0 = zero.X[:, :, 0]
    dev = np.abs(d0 - sx * z0)
    assert np.all(dev <= _draw_bound(sx, z0)), f"{tag}: the start draw is not the definition: {np.max(dev / np.maximum(_draw_bound(sx, z0), 1e-300)):.3g} bounds"
    assert np.all(d0[..., sx == 0.0] == 0.0), f"{tag}: sigma_x0 0 must add nothing"
    with np.errstate(invalid="ignore", divide="ignore"):
        worst["dev"] = max(worst["dev"], float(np.nanmax(np.where(sx > 0, dev / (sx * np.maximum(1.0, np.abs(z0))), 0.0))))
    assert np.array_equal(res[False].X[:, :, 0], plan["X"][:, None, 0, :] + d0), f"{tag}: X[:, :, 0] is not the plan's start + the draw"
    centre = plan["X"][:, None, 0, :] + 0.125 * np.arange(S)[None, :, None]   # a caller's centre
    rc = p.closed_loop_noise(S, seed, None, sx, x0=centre, want_stats=False, want_X=True)
    assert np.array_equal(rc.X[:, :, 0], centre + d0), f"{tag}: X[:, :, 0] is not the caller's centre + the draw"
    # all sigmas 0: the undisturbed call
    n0 = p.closed_loop_noise(S, seed, None, None, want_X=True, want_U=True, want_w=True)
    c0, X0, U0 = p.closed_loop(samples=S)
    assert np.array_equal(n0.cost, c0) and np.array_equal(n0.X, X0) and np.array_equal(n0.U, U0) and not np.any(n0.w), f"{tag}: sigma 0 is not the null call"
    return res[False]


def numpy_stats(cost):
    """[B][5] by the definition, with np.longdouble sums."""
    out = np.empty((cost.shape[0], 5))
    for b, row in enumerate(cost):
        fin = row[np.isfinite(row)].astype(np.longdouble)
        n = len(fin)
        mean = fin.sum() / n if n else np.nan
        var = ((fin - mean) ** 2).sum() / (n - 1) if n > 1 else (0.0 if n else np.nan)
        out[b] = (mean, var, fin.min() if n else np.nan, fin.max() if n else np.nan, len(row) - n)
    return out


def check_stats(stats, cost, tag, need_spread=1e-3):
    """(5) for one call's stats against its own costs.  need_spread: the std / mean every instance must reach for the variance bound to be
    fair (the two-pass error is about 2 * 2^-53 mean / std: 2e-13 at 1e-3).  The time systems may not be given a sigma above 1e-3, and at
    T = 2, 3 their three to five costs then spread by 1e-4 of their mean; they are held to the same 1e-10 with 1e-5 asserted, where that
    error model still gives 2e-11."""
    ref = numpy_stats(cost)
    assert np.array_equal(stats[:, 4], ref[:, 4]), f"{tag}: n_bad {stats[:, 4]} != {ref[:, 4]}"
    assert np.array_equal(stats[:, 2:4], ref[:, 2:4], equal_nan=True), f"{tag}: min / max differ from NumPy's"
    some = ref[:, 4] < cost.shape[1]
    assert np.all(np.isnan(stats[~some, :4])), f"{tag}: no finite sample must give NaN"
    np.testing.assert_allclose(stats[some, 0], ref[some, 0], rtol=1e-12, atol=0, err_msg=f"{tag}: mean")
    many = ref[:, 4] < cost.shape[1] - 1
    if need_spread and np.any(many):   # the two-pass error is about 2 * 2^-53 mean / std: the bound below needs std / mean >= 1e-3
        ratio = np.sqrt(ref[many, 1]) / np.abs(ref[many, 0])
        assert np.all(ratio >= need_spread), f"{tag}: std / mean {ratio.min():.2e} < {need_spread:g}: choose a larger sigma"
    np.testing.assert_allclose(stats[many, 1], ref[many, 1], rtol=1e-10, atol=0, err_msg=f"{tag}: variance")
    one = some & ~many
    assert np.all(stats[one, 1] == 0.0), f"{tag}: a single finite sample has variance 0"


def check_stats_case(p, plan, S, seed, sw, sx, base, tag, spread=1e-3):
    """(5): base = the noise call's result with cost and stats"""
    check_stats(base.stats, base.cost, tag, need_spread=spread)
    only = p.closed_loop_noise(S, seed, sw, sx, want_cost=False)
    assert only.cost is None and np.array_equal(only.stats, base.stats, equal_nan=True), f"{tag}: stats without cost differ from stats with it"


def check_finite_only_rule(p, plan, seed, sw, sx, tag):
    """(5): two non-finite per-sample costs planted through the caller's centre (a NaN start and one of 1e300), plus an instance whose every
    sample is bad and one with a single good sample"""
    Bn, _, nxu = plan["X"].shape
    S = 5
    centre = np.repeat(plan["X"][:, None, 0, :], S, axis=1)
    centre[3, 1, 0] = np.nan
    centre[3, 4, :] = 1e300
    centre[5, :, 0] = np.nan
    centre[7, 1:, 0] = np.nan
    r = p.closed_loop_noise(S, seed, sw, sx, x0=centre)
    bad = ~np.isfinite(r.cost)
    assert bad[3].tolist() == [False, True, False, False, True] and bad[5].all() and bad[7].tolist() == [False] + [True] * 4, f"{tag}: {bad[[3, 5, 7]]}"
    assert bad.sum() == 2 + S + S - 1, f"{tag}: an execution that was not planted is not finite"
    check_stats(r.stats, r.cost, tag, need_spread=0)
    assert r.stats[3, 4] == 2 and r.stats[5, 4] == S and np.all(np.isnan(r.stats[5, :4])) and r.stats[7, 1] == 0.0 and r.stats[7, 0] == r.cost[7, 0]


def check_case(ctx, name, T, samples, seed=SEED, worst=None, compare_generic=False):
    """(1), (2), (5) on one plan for every S of `samples`; compare_generic: (3), the calls under the generic pin return the same bits."""
    cfg, desc, inp, _ = cl.make_case(ctx, name, T)
    worst = worst if worst is not None else dict(dev=0.0)
    p = cl.solve(ctx, cfg, desc, inp)
    try:
        plan = cl.plan_of(p)
        sw, sx = sigma_vectors(plan["X"].shape[2], *scales(name))
        for S in samples:
            tag = f"{name} T={T} S={S}"
            base = check_draw(p, plan, S, seed + S, sw, sx, tag, worst)
            check_stats_case(p, plan, S, seed + S, sw, sx, base, tag, spread=1e-5 if name in cl.TIME_SHAPES else 1e-3)
            if compare_generic:
                for ff in (False, True):
                    a = p.closed_loop_noise(S, seed + S, sw, sx, with_feedforward=ff, want_X=True, want_U=True, want_w=True)
                    with cl.generic_pin():
                        g = p.closed_loop_noise(S, seed + S, sw, sx, with_feedforward=ff, want_X=True, want_U=True, want_w=True)
                    for an, av, gv in zip(a._fields, a, g):
                        assert np.array_equal(av, gv, equal_nan=True), f"{tag} ff={ff}: {an} of the generic kernel differs by {np.abs(av - gv).max():.3e}"
        if name in ("C2", "limits", "C4t1"):
            check_finite_only_rule(p, plan, seed, sw, sx, f"{name} T={T} planted")
    finally:
        p.close()
    return f"{name} T={T} S={tuple(samples)}: worst draw deviation so far {worst['dev']:.3e} sigma max(1, |z|)"


def cut_inputs(inp, bs):
    out = dict(inp)
    for k in ("q0", "dq0", "U0", "lambda0"):
        if k in inp:
            out[k] = np.ascontiguousarray(inp[k][bs])
    out["targets"] = [np.ascontiguousarray(t[bs]) for t in inp["targets"]]
    return out


def check_cut_out(ctx, name):
    """(4): instances 2 .. 10 and samples 1 .. 13 of a 13 x 17 call as a call of their own"""
    T, S = 9, 17
    cfg, desc, inp, _ = cl.make_case(ctx, name, T)
    kw = dict(with_feedforward=True, want_X=True, want_U=True, want_w=True)
    p = cl.solve(ctx, cfg, desc, inp)
    try:
        sw, sx = sigma_vectors(p.dims.n_x, *scales(name))
        big = p.closed_loop_noise(S, SEED, sw, sx, **kw)
        again = p.closed_loop_noise(S, SEED, sw, sx, **kw)
        other = p.closed_loop_noise(S, SEED + 1, sw, sx, **kw)
    finally:
        p.close()
    for f, a, b in zip(big._fields, big, again):
        assert np.array_equal(a, b), f"{name}: {f} differs between two calls with one seed"
    assert np.all(other.cost != big.cost) and np.all(np.any(other.w != big.w, axis=(2, 3))), f"{name}: another seed leaves a sample unchanged"
    bs, ss_ = slice(2, 11), slice(1, 14)
    q = cl.solve(ctx, cfg, desc, cut_inputs(inp, bs))
    try:
        small = q.closed_loop_noise(13, SEED, sw, sx, instance_offset=2, sample_offset=1, **kw)
    finally:
        q.close()
    for f, a, b in zip(big._fields, big, small):
        if f != "stats":
            assert np.array_equal(a[bs, ss_], b), f"{name}: {f} of the cut-out differs from the large call"
    check_stats(small.stats, small.cost, f"{name} cut-out", need_spread=1e-5 if name in cl.TIME_SHAPES else 1e-3)


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def check_stream(z, tag):
    """(6): z[B][S][K][n] standard normals.  Returns the z-scores."""
    n = z.size
    zs = dict(mean=z.mean() * np.sqrt(n), var=(z.var() - 1.0) / np.sqrt(2.0 / n))
    pairs = dict(entries=(z[..., 0], z[..., 1]), samples=(z[:, :-1], z[:, 1:]), instances=(z[:-1], z[1:]), steps=(z[:, :, :-1], z[:, :, 1:]))
    for k, (a, b) in pairs.items():
        zs["corr_" + k] = _corr(a, b) * np.sqrt(a.size)
    for k, v in zs.items():
        assert abs(v) < 4.0, f"{tag}: {k} is {v:.2f} standard errors from its expectation"
    return zs


def check_stream_of_call(ctx):
    """(6) on the restatement, then on w_out / sigma of one C2 call with B = 13, S = 17, T = 9, seed 12345"""
    T, S = 9, 17
    zr = draw(SEED, cl.B, S, range(T - 1), 7)
    out = [check_stream(zr, "restatement")]
    cfg, desc, inp, _ = cl.make_case(ctx, "C2", T)
    p = cl.solve(ctx, cfg, desc, inp)
    try:
        sig = 1e-3 * (1.0 + np.arange(7))
        r = p.closed_loop_noise(S, SEED, sig, None, want_w=True)
    finally:
        p.close()
    out.append(check_stream(r.w / sig, "w_out / sigma"))
    assert np.allclose(r.w / sig, zr, rtol=0, atol=1e-13)
    return out


def refused(call, text):
    cl._refused(call, text)


def check_interfaces(ctx, device_call):
    """(8): every refusal by its text, before any launch; the _dev entry point equals the host one.
    device_call(p, S, nz, x0, ff) -> (cost, stats, X, U, w) through ilqr_problem_closed_loop_noise_dev."""
    import ctypes as C

    from ilqr_planner_amd import workloads

    cfg, desc, inp, _ = cl.make_case(ctx, "C2", 9)
    p = workloads.load_batch(ctx, desc, inp, cl.B)
    try:
        refused(lambda: p.closed_loop_noise(2, 1, 1e-3), "closed loop needs the gains")
        workloads.run_solver(p, cfg, nb_iter=cl.NIT, early_stop=True)
        refused(lambda: p.closed_loop_noise(0, 1, 1e-3), "n_samples must be >= 1")
        dp = C.POINTER(C.c_double)
        one = np.zeros(cl.B * 5)
        raw = lambda S, nz, cost, stats, X=None: ctx.check(p.L.ilqr_problem_closed_loop_noise(  # noqa: E731
            p.h, S, nz, None, 0, cost.ctypes.data_as(dp) if cost is not None else None, stats.ctypes.data_as(dp) if stats is not None else None,
            X.ctypes.data_as(dp) if X is not None else None, None, None))
        refused(lambda: raw(1, None, one, None), "noise is a null pointer")
        for bad in (-1e-3, np.nan, np.inf):
            refused(lambda: p.closed_loop_noise(2, 1, bad), "sigma_w and sigma_x0 must be finite and >= 0")
            refused(lambda: p.closed_loop_noise(2, 1, None, [0, 0, bad, 0, 0, 0, 0]), "sigma_w and sigma_x0 must be finite and >= 0")
        refused(lambda: p.closed_loop_noise(2, 1, 1e-3, want_cost=False, want_stats=False), "cost and stats are both null pointers")
        refused(lambda: p.closed_loop_noise(2, 1, 1e-3, instance_offset=2 ** 32 - cl.B + 1), "exceeds 2^32")
        refused(lambda: p.closed_loop_noise(2, 1, 1e-3, sample_offset=2 ** 32 - 1), "exceeds 2^32")
        assert p.closed_loop_noise(2, 1, 1e-3, instance_offset=2 ** 32 - cl.B, sample_offset=2 ** 32 - 2).stats.shape == (cl.B, 5)
        nz = p.noise(1, 1e-3)
        nx = p.dims.n_x
        big_steps = (1 << 31) // (cl.B * 9 * nx) + 1     # too many for a per-step array, fine without one
        refused(lambda: raw(big_steps, C.byref(nz), one, None, X=one), "B * n_samples * T * n_x overflows the kernels' 32-bit offsets")
        big = (1 << 31) // (cl.B * nx) + 1
        refused(lambda: raw(big, C.byref(nz), one, None), "B * n_samples * n_x overflows the kernels' 32-bit offsets")
        sw, sx = sigma_vectors(nx, 1e-3, 1e-2)
        x0 = cl.plan_of(p)["X"][:, None, 0, :] + np.zeros((1, 5, 1))
        for centre in (None, x0):
            host = p.closed_loop_noise(5, 9, sw, sx, x0=centre, with_feedforward=True, want_X=True, want_U=True, want_w=True)
            dev = device_call(p, 5, p.noise(9, sw, sx), centre, True)
            for f, h, d in zip(host._fields, host, dev):
                assert np.array_equal(h, d), f"{f} of the device-pointer entry point differs from the host one"
        p.set_controls(inp["U0"])
        refused(lambda: p.closed_loop_noise(2, 1, 1e-3), "closed loop needs the gains")
    finally:
        p.close()


def host_pointer_call(p, S, nz, x0, ff):
    """ilqr_problem_closed_loop_noise_dev on arrays of the host: what a device pointer is on the host build of the kernels"""
    T, nx, nu = p.T, p.dims.n_x, p.dims.n_u
    x0 = np.ascontiguousarray(x0) if x0 is not None else None
    cost, stats = np.zeros((p.B, S)), np.zeros((p.B, 5))
    X, U, w = np.zeros((p.B, S, T, nx)), np.zeros((p.B, S, T - 1, nu)), np.zeros((p.B, S, T - 1, nx))
    p.closed_loop_noise_dev(S, nz, x0.ctypes.data if x0 is not None else None, ff, cost.ctypes.data, stats.ctypes.data, X.ctypes.data, U.ctypes.data,
                            w.ctypes.data)
    p.ctx.synchronize()
    stats_only = np.zeros((p.B, 5))
    p.closed_loop_noise_dev(S, nz, x0.ctypes.data if x0 is not None else None, ff, None, stats_only.ctypes.data)   # the costs in the problem's workspace
    p.ctx.synchronize()
    assert np.array_equal(stats_only, stats)
    return cost, stats, X, U, w
