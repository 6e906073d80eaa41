"""Analytic covariance of the closed loop (ilqr_problem_closed_loop_cov) -- the checks shared by tests/tools/hostsim/closed_loop_cov_checks.py
(host build of the generic kernel k_cl_cov) and tests/test_gpu_closed_loop_cov.py (k_cl_cov_rows and, under the pin, k_cl_cov on the device).
Cases and plans come from tests/closed_loop.py.

  (1) Sigma, kp_Sigma, u_var, lim_z against the recursion Sigma' = F Sigma F' + diag(sigma_w^2) in NumPy on the getters' X, U, K, with A, B
      written here from the formulas of include/ilqr_hip.h; kp_var with the Jacobian of ilqr_fk_batch.  Bound: closed_loop._within,
      1e-9 max(1, |.|_inf); where an output of an instance misses it, its deviation may be at most ILL_FACTOR times what the recursion itself
      moves when run in np.longdouble (counted).
  (2) A, B are the Jacobian of the oracle's step: central differences at two widths h, h / 2.  The step is a cubic polynomial, so the error
      of the narrower one is a third of their difference; the bound is that difference plus the rounding of a difference quotient,
      8 eps max(1, |f|_inf) / (h / 2).  The reference's own time column (velocity after the step) must miss that bound on PosOrnTime-2.
  (3) exact properties, array_equal: Sigma_0 = diag(sigma_x0^2); symmetry; zero sigmas; doubling the sigmas; subsets of the outputs; cut-outs;
      host pointers = device pointers.
  (4) the sample covariance of closed_loop_noise's X within 6 sampling standard deviations of Sigma (constant-dt systems), with power.
  (5) refusals and interfaces.
"""
from __future__ import annotations

import itertools

import numpy as np

from ilqr_planner_amd import workloads
from tests import closed_loop as cl
from tests import closed_loop_noise as cn
from tests.helpers import orc

HORIZONS = (2, 3, 9, 25)
FIELDS = ("Sigma", "kp_Sigma", "kp_var", "u_var", "lim_z")
SAMPLED = ("C2", "C2nd", "C1j")   # PosOrn-1, PosOrn-2, JointSpace: constant dt, the recursion is exact
FD_H = 1e-3


def dims_of(kind, nd, nxu):
    tm = 1 if kind in (1, 3) else 0
    return (nxu - tm) // nd, tm


def jacobian(kind, nd, dt, x, u, ld=np.float64, quirk=False):
    """A [n_x][n_x], B [n_x][n_u] of the step at (x, u) in the user's layout [q | v | t].  quirk: the reference's time column on the position
    rows of a 2nd-order system (the velocity after the step), which is not the Jacobian."""
    nx = len(x)
    dof, tm = dims_of(kind, nd, nx)
    x, u = np.asarray(x, dtype=ld), np.asarray(u, dtype=ld)
    A, B = np.eye(nx, dtype=ld), np.zeros((nx, dof + tm), dtype=ld)
    dts = u[-1] if tm else None
    h = dts * dts if tm else ld(dt)
    I = np.arange(dof)
    if nd == 1:
        B[I, I] = h
    else:
        A[I, dof + I] = h
        B[I, I] = h * h / 2
        B[dof + I, I] = h
    if tm:
        if nd == 1:
            B[I, -1] = 2 * dts * u[:dof]
        else:
            v = x[dof:2 * dof] + (h * u[:dof] if quirk else 0)
            B[I, -1] = 2 * dts * v + 2 * dts ** 3 * u[:dof]
            B[dof + I, -1] = 2 * dts * u[:dof]
        B[-1, -1] = 2 * dts
    return A, B


def recursion(kind, nd, dt, X, U, K, sw, sx, ld=np.float64, open_loop=False):
    """(Sigma [T][n_x][n_x], u_var [T-1][n_u]) of one instance"""
    T, nx = X.shape
    sw, sx = np.asarray(sw, dtype=ld), np.asarray(sx, dtype=ld)
    Sg, uv = np.zeros((T, nx, nx), dtype=ld), np.zeros((T - 1, U.shape[1]), dtype=ld)
    Sg[0] = np.diag(sx * sx)
    for k in range(T - 1):
        A, B = jacobian(kind, nd, dt, X[k], U[k], ld)
        Kk = np.zeros_like(K[k], dtype=ld) if open_loop else K[k].astype(ld)
        F = A + B @ Kk
        uv[k] = np.einsum("ij,jk,ik->i", Kk, Sg[k], Kk)
        Sn = F @ Sg[k] @ F.T + np.diag(sw * sw)
        Sg[k + 1] = (Sn + Sn.T) / 2
    return Sg, uv


def limit_sets(desc, nxu):
    """[(smax, smin, weighted)] of the descriptor's limit sets in the user's state layout"""
    out = []
    if desc.limits_set:
        out.append((np.array(desc.state_max[:nxu]), np.array(desc.state_min[:nxu]), np.array(desc.limit_weight[:nxu]) != 0))
    if desc.limits2_set:
        out.append((np.array(desc.state_max2[:nxu]), np.array(desc.state_min2[:nxu]), np.array(desc.limit_weight2[:nxu]) != 0))
    return out


def lim_z_of(sets, X, Sg):
    z = np.inf
    d = np.einsum("kii->ki", Sg)
    for smax, smin, on in sets:
        m = on[None, :] & (d > 0)
        if m.any():
            with np.errstate(divide="ignore", invalid="ignore"):
                q = np.minimum(smax - X, X - smin) / np.sqrt(np.where(m, d, 1))
            z = min(z, float(q[m].min()))
    return z


def kp_var_of(kind, nd, kp_joint, J, Sg):
    """[5] of one keypoint: J [6][dof] (None for a joint keypoint), Sg = Sigma at its step"""
    nx = Sg.shape[0]
    dof, tm = dims_of(kind, nd, nx)
    v = np.zeros(5, dtype=Sg.dtype)
    if kind in (2, 3) or kp_joint:
        v[0] = np.trace(Sg[:dof, :dof])
    else:
        J = J.astype(Sg.dtype)
        for blk in range(nd):
            C = J @ Sg[blk * dof:(blk + 1) * dof, blk * dof:(blk + 1) * dof] @ J.T
            v[2 * blk], v[2 * blk + 1] = np.trace(C[:3, :3]), np.trace(C[3:, 3:])
    if tm:
        v[4] = Sg[-1, -1]
    return v


def reference(ctx, cfg, desc, plan, sw, sx, ld=np.float64, open_loop=False):
    """dict of the five outputs by the NumPy recursion"""
    kind, nd = desc.kind, desc.nb_deriv
    X, U, K = plan["X"], plan["U"], plan["K"]
    Bn, T, nx = X.shape
    dof, _ = dims_of(kind, nd, nx)
    n_kp = int(desc.n_kp)
    kt = [int(desc.kp_timestep[k]) for k in range(n_kp)]
    sets = limit_sets(desc, nx)
    Sg, uv, lz = np.zeros((Bn, T, nx, nx), dtype=ld), np.zeros((Bn, T - 1, U.shape[2]), dtype=ld), np.zeros(Bn)
    kv = np.zeros((Bn, n_kp, 5), dtype=ld)
    for b in range(Bn):
        Sg[b], uv[b] = recursion(kind, nd, cfg.get("dt"), X[b], U[b], K[b], sw, sx, ld, open_loop)
        lz[b] = lim_z_of(sets, X[b], Sg[b].astype(np.float64))
    for k in range(n_kp):
        J = None
        if kind in (0, 1) and not desc.kp_joint[k]:
            J = ctx.fk_batch(desc, np.ascontiguousarray(X[:, kt[k], :dof]))[2]
        for b in range(Bn):
            kv[b, k] = kp_var_of(kind, nd, bool(desc.kp_joint[k]), None if J is None else J[b], Sg[b, kt[k]])
    return dict(Sigma=Sg, kp_Sigma=Sg[:, kt] if n_kp else np.zeros((Bn, 0, nx, nx), dtype=ld), kp_var=kv, u_var=uv, lim_z=lz)


def new_stats():
    return dict(n=0, ill=0, worst_ratio=0.0, **{f: 0.0 for f in FIELDS})


def _flat(a, b):
    a = np.asarray(a[b], dtype=np.float64)
    return a.reshape(1, -1) if a.ndim <= 1 else a.reshape(-1, a.shape[-1])


def check_against_recursion(ctx, cfg, desc, plan, sw, sx, got, tag, stats):
    """(1)"""
    ref = reference(ctx, cfg, desc, plan, sw, sx)
    wide = None
    for b in range(plan["X"].shape[0]):
        for f in FIELDS:
            g, r = _flat(getattr(got, f), b), _flat(ref[f], b)
            assert g.shape == r.shape, f"{tag}: {f} has shape {getattr(got, f).shape}"
            if g.size == 0:
                continue
            assert not np.any(np.isnan(g)), f"{tag}: {f}[{b}] holds NaN"
            stats["n"] += 1
            inf = np.isinf(r)
            assert np.array_equal(g[inf], r[inf]), f"{tag}: {f}[{b}] is {g[inf]} where the recursion gives {r[inf]}"
            g, r = np.where(inf, 0.0, g), np.where(inf, 0.0, r)
            dev = float(np.abs(g - r).max())
            if cl._within(g, r):
                stats[f] = max(stats[f], dev)
                continue
            wide = wide if wide is not None else reference(ctx, cfg, desc, plan, sw, sx, ld=np.longdouble)
            ww = _flat(wide[f], b)
            sens = float(np.abs(np.where(inf, 0.0, ww) - r).max())
            assert dev <= cl.ILL_FACTOR * sens, f"{tag}: {f}[{b}] is {dev:.3e} from the recursion, which np.longdouble moves by {sens:.3e}"
            stats["ill"] += 1
            stats["worst_ratio"] = max(stats["worst_ratio"], dev / sens)


def fd_jacobian(s, x, u, h):
    cols = []
    for j in range(len(x) + len(u)):
        e = np.zeros(len(x) + len(u))
        e[j] = h
        hi = orc.step(s, x + e[:len(x)], u + e[len(x):])[0]
        lo = orc.step(s, x - e[:len(x)], u - e[len(x):])[0]
        cols.append((hi - lo) / (2 * h))
    return np.stack(cols, axis=1)


def check_jacobian(systems, cfg, desc, plan, tag):
    """(2) at the plan points (x_k, u_k), k = 0 and T - 2, of the first three instances"""
    kind, nd = desc.kind, desc.nb_deriv
    T = plan["X"].shape[1]
    worst, n_quirk = 0.0, 0
    for b in range(3):
        for k in sorted({0, T - 2}):
            x, u = plan["X"][b, k], plan["U"][b, k]
            D1, D2 = fd_jacobian(systems[b], x, u, FD_H), fd_jacobian(systems[b], x, u, FD_H / 2)
            fmax = max(1.0, float(np.abs(orc.step(systems[b], x, u)[0]).max()))
            bound = np.abs(D1 - D2) + 8 * np.finfo(np.float64).eps * fmax / (FD_H / 2)
            AB = np.hstack(jacobian(kind, nd, cfg.get("dt"), x, u))
            miss = np.abs(AB - D2) - bound
            assert np.all(miss <= 0), f"{tag} b={b} k={k}: [A B] is {np.abs(AB - D2).max():.3e} from the oracle's step, entry {np.unravel_index(miss.argmax(), miss.shape)}"
            worst = max(worst, float(np.abs(AB - D2).max()))
            if kind == 1 and nd == 2 and abs(u[-1]) > 1e-3 and np.abs(u[:-1]).max() > 1e-3:
                ABq = np.hstack(jacobian(kind, nd, cfg.get("dt"), x, u, quirk=True))
                assert np.any(np.abs(ABq - D2) > bound), f"{tag} b={b} k={k}: the velocity after the step passes as the Jacobian"
                n_quirk += 1
    assert not (kind == 1 and nd == 2) or n_quirk > 0, f"{tag}: no plan point had controls large enough to tell the two time columns apart"
    return worst


def call(p, sw, sx, **kw):
    return p.closed_loop_cov(sw, sx, want_Sigma=True, **kw)


def check_exact(p, plan, sw, sx, full, tag):
    """(3) on one plan, without the cut-out and the device pointers"""
    Bn, T, nx = plan["X"].shape
    assert np.array_equal(full.Sigma[:, 0], np.broadcast_to(np.diag(sx * sx), (Bn, nx, nx))), f"{tag}: Sigma_0 is not diag(sigma_x0^2)"
    assert np.array_equal(full.Sigma, np.swapaxes(full.Sigma, 2, 3)), f"{tag}: Sigma is not symmetric"
    assert np.array_equal(full.kp_Sigma, np.swapaxes(full.kp_Sigma, 2, 3)), f"{tag}: kp_Sigma is not symmetric"
    for zero in (call(p, None, None), call(p, 0.0, np.zeros(nx))):
        for f in FIELDS[:4]:
            assert not np.any(getattr(zero, f)), f"{tag}: zero sigmas give a non-zero {f}"
        assert np.all(zero.lim_z == np.inf), f"{tag}: zero sigmas give lim_z {zero.lim_z}"
    twice = call(p, 2 * sw, 2 * sx)
    for f in FIELDS[:4]:
        assert np.array_equal(getattr(twice, f), 4 * getattr(full, f)), f"{tag}: doubled sigmas do not multiply {f} by exactly 4"
    assert np.array_equal(twice.lim_z, full.lim_z / 2), f"{tag}: doubled sigmas do not halve lim_z exactly"
    for n in range(1, 5):
        for keep in itertools.combinations(FIELDS, n):
            part = p.closed_loop_cov(sw, sx, **{"want_" + f: f in keep for f in FIELDS})
            for f in FIELDS:
                a = getattr(part, f)
                assert (a is None) == (f not in keep)
                assert a is None or np.array_equal(a, getattr(full, f)), f"{tag}: {f} of the call for {keep} differs from the all-outputs call"


def sigmas(nx):
    """sigma_w, sigma_x0: graded, with zero entries (cn.sigma_vectors), 1e-3 and 1e-2 at the most"""
    return cn.sigma_vectors(nx, 1e-3, 1e-2)


def check_case(ctx, name, T, stats=None, pins=(False,), jac_worst=None):
    """(1), (2), (3) on one plan; pins: for each, the checks run under the generic pin (True) or with the planned kernel (False)."""
    cfg, desc, inp, systems = cl.make_case(ctx, name, T)
    stats = stats if stats is not None else new_stats()
    n0, ill0 = stats["n"], stats["ill"]
    p = cl.solve(ctx, cfg, desc, inp)
    try:
        plan = cl.plan_of(p)
        assert all(np.all(np.isfinite(plan[f])) for f in ("X", "U", "K")), f"{name} T={T}: the plan is not finite"
        sw, sx = sigmas(plan["X"].shape[2])
        w = check_jacobian(systems, cfg, desc, plan, f"{name} T={T}")
        if jac_worst is not None:
            jac_worst[0] = max(jac_worst[0], w)
        res = []
        for pin in pins:
            tag = f"{name} T={T}" + (" generic" if pin else "")
            with (cl.generic_pin() if pin else _nothing()):
                full = call(p, sw, sx)
                check_against_recursion(ctx, cfg, desc, plan, sw, sx, full, tag, stats)
                check_exact(p, plan, sw, sx, full, tag)
            res.append(full)
        if len(res) == 2:   # the two kernels agree to rounding: each is within (1) of the recursion; here, that the pin reached another kernel or not
            same = all(np.array_equal(getattr(res[0], f), getattr(res[1], f)) for f in FIELDS)
            stats["same" if same else "differ"] = stats.get("same" if same else "differ", 0) + 1
    finally:
        p.close()
    return f"{name} T={T}: {stats['n'] - n0} outputs, {stats['ill'] - ill0} by their sensitivity"


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def check_cut_out(ctx, name, T=9):
    """(3): instances 2 .. 10 as a problem of their own reproduce the large call's bits"""
    cfg, desc, inp, _ = cl.make_case(ctx, name, T)
    bs = slice(2, 11)
    p = cl.solve(ctx, cfg, desc, inp)
    try:
        sw, sx = sigmas(p.dims.n_x)
        big = call(p, sw, sx)
    finally:
        p.close()
    q = cl.solve(ctx, cfg, desc, cn.cut_inputs(inp, bs))
    try:
        small = call(q, sw, sx)
    finally:
        q.close()
    for f in FIELDS:
        assert np.array_equal(getattr(big, f)[bs], getattr(small, f)), f"{name}: {f} of the cut-out differs from the large call"


def check_sampled(ctx, name, S=4096, T=9, Bn=3, seed=2024):
    """(4).  Returns the largest |sample covariance - Sigma| in sampling standard deviations."""
    cfg, desc, inp, _ = cl.make_case(ctx, name, T)
    p = cl.solve(ctx, cfg, desc, cn.cut_inputs(inp, slice(0, Bn)))
    try:
        plan = cl.plan_of(p)
        nx = plan["X"].shape[2]
        sg = np.full(nx, 1e-3)
        X = p.closed_loop_noise(S, seed, sg, sg, want_stats=False, want_X=True).X
        Sg = call(p, sg, sg).Sigma
        open_loop = reference(ctx, cfg, desc, plan, sg, sg, open_loop=True)["Sigma"]
    finally:
        p.close()
    assert np.all(np.isfinite(X))
    worst, worst_open = 0.0, 0.0
    for b in range(Bn):
        for k in range(T):
            C = np.cov(X[b, :, k, :], rowvar=False, ddof=1).reshape(nx, nx)
            for M, is_open in ((Sg[b, k], False), (open_loop[b, k], True)):
                dg = np.diag(M)
                sd = np.sqrt((np.outer(dg, dg) + M * M) / (S - 1))
                ratio = float((np.abs(C - M) / sd).max())
                if is_open:
                    worst_open = max(worst_open, ratio)
                else:
                    worst = max(worst, ratio)
                    assert ratio <= 6.0, f"{name} b={b} k={k}: the sample covariance is {ratio:.2f} standard deviations from Sigma"
    assert worst_open > 6.0, f"{name}: the open-loop recursion passes too ({worst_open:.2f}): the check has no power"
    return worst, worst_open


def check_interfaces(ctx, device_call, batch_solver=False, size_refusals=False):
    """(5): every refusal by its text; the _dev entry point returns what the host one does.
    device_call(p, sw, sx, wants: dict field -> bool) -> ClosedLoopCov through ilqr_problem_closed_loop_cov_dev."""
    import ctypes as C

    from ilqr_planner_amd import capi

    cfg, desc, inp, _ = cl.make_case(ctx, "C2", 9)
    p = workloads.load_batch(ctx, desc, inp, cl.B)
    try:
        cl._refused(lambda: p.closed_loop_cov(1e-3), "closed loop needs the gains")
        p.solve_recursive(0, True, False)
        cl._refused(lambda: p.closed_loop_cov(1e-3), "closed loop needs the gains")
        solve_again = lambda: workloads.run_solver(p, cfg, nb_iter=cl.NIT, early_stop=True)  # noqa: E731
        solve_again()
        for bad in (-1e-3, np.nan, np.inf):
            cl._refused(lambda: p.closed_loop_cov(bad), "sigma_w and sigma_x0 must be finite and >= 0")
            cl._refused(lambda: p.closed_loop_cov(None, [0, 0, bad, 0, 0, 0, 0]), "sigma_w and sigma_x0 must be finite and >= 0")
        cl._refused(lambda: ctx.check(p.L.ilqr_problem_closed_loop_cov(p.h, None, None, None)), "every output is a null pointer")
        cl._refused(lambda: p.closed_loop_cov(1e-3, want_kp_Sigma=False, want_kp_var=False, want_u_var=False, want_lim_z=False),
                    "every output is a null pointer")
        sw, sx = sigmas(p.dims.n_x)
        host = call(p, sw, sx)
        for keep in (FIELDS, ("kp_var",), ("Sigma", "lim_z"), ("kp_Sigma", "u_var")):
            wants = {f: f in keep for f in FIELDS}
            dev = device_call(p, sw, sx, wants)
            for f in FIELDS:
                assert (getattr(dev, f) is None) == (not wants[f])
                assert not wants[f] or np.array_equal(getattr(dev, f), getattr(host, f)), f"{f} of the device-pointer entry point differs from the host one"
        if batch_solver:
            p.solve_batch(1)
            cl._refused(lambda: p.closed_loop_cov(1e-3), "closed loop needs the gains")
            solve_again()
            assert np.array_equal(call(p, sw, sx).Sigma, host.Sigma)
        p.set_controls(inp["U0"])
        cl._refused(lambda: p.closed_loop_cov(1e-3), "closed loop needs the gains")
    finally:
        p.close()
    if not size_refusals:
        return
    # The bounds and their texts are cl_cov_size_refusal's, checked on the host at every size (tests/cpp/closed_loop_cov_plan_main.cpp).  Here, that the
    # entry point asks it before every other refusal, allocation and launch: an unsolved C4 problem (n_x = 15) at T = 25 on 2^31 / (25 * 225) + 1
    # instances.  The kp_Sigma bound through the C ABI would need a problem of a dozen times that size and is left to the host test.
    one = np.zeros(1)
    cfg, desc, inp, _ = cl.make_case(ctx, "C4", 25)
    big = capi.BatchProblem(ctx, desc, (1 << 31) // (25 * 225) + 1)
    try:
        cv = capi.Cov(Sigma=one.ctypes.data)
        cl._refused(lambda: ctx.check(big.L.ilqr_problem_closed_loop_cov(big.h, None, None, C.byref(cv))), "B * T * n_x^2 reaches 2^31")
        cv = capi.Cov(lim_z=one.ctypes.data)   # without Sigma the size is fine, and the next refusal answers
        cl._refused(lambda: ctx.check(big.L.ilqr_problem_closed_loop_cov(big.h, None, None, C.byref(cv))), "closed loop needs the gains")
    finally:
        big.close()


def host_pointer_call(p, sw, sx, wants):
    """ilqr_problem_closed_loop_cov_dev on arrays of the host: what a device pointer is on the host build of the kernels"""
    from ilqr_planner_amd import capi

    nx, nk = p.dims.n_x, p.n_kp
    shapes = dict(Sigma=(p.B, p.T, nx, nx), kp_Sigma=(p.B, nk, nx, nx), kp_var=(p.B, nk, 5), u_var=(p.B, p.T - 1, p.dims.n_u), lim_z=(p.B,))
    out = {f: (np.zeros(shapes[f]) if wants[f] else None) for f in FIELDS}
    p.closed_loop_cov_dev(sw, sx, **{f + "_ptr": (out[f].ctypes.data if out[f] is not None else None) for f in FIELDS})
    p.ctx.synchronize()
    return capi.ClosedLoopCov(**out)
