"""AL-iLQR at every constraint-row capacity, multipliers included -- shared by tests/test_gpu_al_shapes.py (the device kernels),
tests/test_al_shapes_cpu.py (the oracle-only conditions) and tests/tools/hostsim/al_shape_checks.py (the host build of the generic kernels).

The number of inequality rows m decides which sweep runs and how it holds the rows (csrc/ilqr_plan.hpp): up to 4 shared state-only rows in the
registers of k_backward_si_dpp, up to 16 rows in the LDS of k_backward_mfma or one per lane of an instance's group in k_backward_rows, anything
else in the generic sweep with its workspace.  The workloads carry one row (q_6 <= bound), so the constraint sets here are made for the tests:
m rows that BIND for some instances of a batch and not for others, on positions, velocities, the time state and the controls.

The non-fused instantiations of k_backward_si_dpp (FUSED = false) run only with alpha_floor < 2^-15 (more than 16 step sizes: the generic
forward pass); tests/solver_constants.py runs them, the 4-row state-only set made here included, against the oracle with the same floor."""
from __future__ import annotations

import numpy as np

from ilqr_planner_amd import workloads
from tests import horizons as hz
from tests import parity_proof as pp
from tests.helpers import oracle_solve_instance, panda_segs

B = hz.B     # 13: ragged on every path
NIT = 6      # iterations of the gated solve: with lag 2 it contains three multiplier updates
LAG = 2
LAYOUTS = ("state", "dense", "control")
X_TOL, U_TOL = 2e-4, 2e-3  # what horizons.check_case allows the trajectories of an instance on the oracle's path


C2R_DIAG = workloads.config("C2r")["R_diag"]  # joint-dependent control weights: the general form of the register-resident sweep, plain gain records
REGISTER_HORIZONS = (25,)                      # (T = 40 as well took the module past the wall time of tests/test_gpu_horizons.py: left out as planned for that case)
RESIDUE_HORIZONS = tuple(range(2, 15))        # every residue of T - 2 modulo 3 and 4, every horizon below a ring
# (system, T) pairs the residue cases leave out because binds() cannot hold there: at T = 2 a row has the one step k = 0 to bind on, where the
# velocities of the 2nd-order systems are zero for every instance (7 of the 16 rows never bind)
RESIDUE_DROPPED = (("C2ndal", 2), ("C4al", 2))
# seeds of the dense rows where the default draw misses binds() (a drawn row is violated by every instance of the batch, or by none)
SEEDS = {("C4t1al", 2, "dense", 25): 1, ("C4al", 17, "dense", 25): 1}


def _case(name, pin, m, layout="state", per_step=False, T=25, R=False):
    return dict(name=name, pin=pin, m=m, layout=layout, per_step=per_step, T=T, R=R)


def case_id(c):
    return f"{c['name']}{'+R' if c['R'] else ''}-{c['pin']}-m{c['m']}-{c['layout']}{'-per_step' if c['per_step'] else ''}-T{c['T']}"


def cases(test):
    """The device matrix of tests/test_gpu_al_shapes.py, one list of cases per test (tests/test_al_shapes_cpu.py asserts binds() for every one).
    A pin is a key of tests/test_gpu_horizons.PINS.  PosOrn-1 (C3) and JointSpace-1 (C1jal) take k_backward_si_dpp up to 4 shared state-only rows
    whatever the pin says; above that, or with control / per-step rows, PosOrn-1 reaches the matrix-core sweep and JointSpace-1 the generic one."""
    out = []
    if test == "register_rows":
        for name, pin, R in (("C3", "dpp", False), ("C3", "wg", False), ("C3", "dpp", True), ("C1jal", "default", False)):
            for T in REGISTER_HORIZONS:
                out += [_case(name, pin, m, "state", T=T, R=R) for m in (1, 2, 3, 4)] + [_case(name, pin, m, "dense", T=T, R=R) for m in (2, 4)]
    elif test == "register_rows_overflow":
        for name in ("C3", "C1jal"):
            out += [_case(name, "default", 5), _case(name, "default", 2, "control"), _case(name, "default", 4, "control"),
                    _case(name, "default", 4, per_step=True)]
    elif test == "lds_rows":
        lds = [("C2ndal", "mfma"), ("C2ndal", "rows")] + [(n, pin) for n in ("C4t1al", "C4al", "C1tal") for pin in ("mfma-dpp", "rows-rows")]
        for name, pin in lds + [("C3", "default")]:
            for m in (2, 15, 16):
                if name == "C3" and m == 2:
                    continue  # (the register-resident sweep: register_rows)
                out += [_case(name, pin, m, "state"), _case(name, pin, m, "dense")]
            out += [_case(name, pin, 16, "control"), _case(name, pin, 16, per_step=True)]
    elif test == "lds_rows_overflow":
        for name in ("C2ndal", "C4t1al", "C4al", "C1tal", "C3"):
            for pin in ("default", "v1"):
                out += [_case(name, pin, 17), _case(name, pin, 32), _case(name, pin, 17, per_step=True)]
    elif test == "rows_at_ring_residues":
        for name, pin, m in (("C3", "dpp", 4), ("C2ndal", "rows", 16), ("C4al", "mfma-dpp", 16)):
            out += [_case(name, pin, m, T=T) for T in RESIDUE_HORIZONS if (name, T) not in RESIDUE_DROPPED]
    elif test == "generic_pin":
        for name in ("C3", "C4al"):
            out += [_case(name, "v1", m, "dense", T=T) for m in (4, 16) for T in (9, 25)]
    else:
        raise KeyError(test)
    return out


TESTS = ("register_rows", "register_rows_overflow", "lds_rows", "lds_rows_overflow", "rows_at_ring_residues", "generic_pin")


def make(ctx, c):
    return make_case(ctx, c["name"], c["T"], c["m"], c["layout"], c["per_step"], R_diag=C2R_DIAG if c["R"] else None,
                     seed=SEEDS.get((c["name"], c["m"], c["layout"], c["T"]), 0))


def make_rows(n_x, n_u, m, layout, rng):
    """A [m][n_x + n_u] of the row layout:
    state    unit rows +-e_j on the states, row r on state r mod n_x, the sign flipping on every wrap (beyond 2 n_x rows a row repeats an
             earlier one: two rows active on one state are legitimate for a penalty method)
    dense    as state, but rows 1, 4, 7, .. have all n_x state coefficients drawn from U(-1, 1)
    control  rows 0 and 1 are +e on the first control and -e on the last one (the time control of a time system: a lower bound on the step
             length), the others as state"""
    assert layout in LAYOUTS, layout
    A = np.zeros((m, n_x + n_u))
    for r in range(m):
        A[r, r % n_x] = -1.0 if (r // n_x) % 2 else 1.0
        if layout == "dense" and r % 3 == 1:
            A[r, :n_x] = rng.uniform(-1.0, 1.0, n_x)
    if layout == "control":
        A[:2] = 0.0
        A[0, n_x] = 1.0
        if m > 1:
            A[1, n_x + n_u - 1] = -1.0
    return A


def _unconstrained(cfg, inp, nb_iter, segs):
    """The oracle's unconstrained solves of the batch (same iteration count, same U0): [(X, U) or None where not finite]."""
    rec = dict(cfg, solver="recursive")
    out = []
    for i in range(len(inp["q0"])):
        r = oracle_solve_instance(rec, inp, i, nb_iter, True, segs)
        out.append((r["X"], r["U"]) if np.all(np.isfinite(r["X"])) and np.all(np.isfinite(r["U"])) else None)
    return out


def make_case(ctx, name, T, m, layout="state", per_step=False, R_diag=None, seed=0, nb_iter=NIT):
    """(cfg, desc, inp) of AL workload `name` at horizon T (horizons.make_case) with m rows of `layout` in place of the workload's one.
    b_r is the batch median of max_k a_r . [x_k; u_k] over the oracle's unconstrained solve of each instance, so that a row binds for
    about half the batch; the multipliers start at zero; the update runs every LAG iterations.  per_step: one constraint set per step,
    the same rows with b_k = b + 0.002 k.  R_diag: control weights in place of the workload's (joint-dependent ones take the general
    form of the register-resident sweep)."""
    cfg, desc, inp = hz.make_case(ctx, name, T)
    assert cfg["solver"] == "al", name
    cfg["al"] = dict(cfg["al"], lag=LAG)
    if R_diag is not None:
        cfg["R_diag"] = list(R_diag)
        for j, v in enumerate(workloads.control_weights(cfg, inp["U0"].shape[2])):
            desc.R_diag[j] = v
    n = inp["A"].shape[1]
    n_u = inp["U0"].shape[2]
    n_x = n - n_u
    A = make_rows(n_x, n_u, m, layout, np.random.default_rng(1000 * m + T + seed))
    mx = []
    for tr in _unconstrained(cfg, inp, nb_iter, panda_segs()):
        if tr is not None:
            Z = np.concatenate([tr[0][: T - 1], tr[1]], axis=1)  # [T-1][n]
            mx.append(np.max(Z @ A.T, axis=0))
    assert mx, f"{name} T={T}: no finite unconstrained solve to take the bounds from"
    b = np.median(np.asarray(mx), axis=0)
    if per_step:
        A = np.ascontiguousarray(np.tile(A, (T - 1, 1, 1)))
        b = np.tile(b, (T - 1, 1)) + 0.002 * np.arange(T - 1)[:, None]
    inp = dict(inp, A=A, b=b, lambda0=np.zeros((len(inp["q0"]), T - 1, m)))
    return cfg, desc, inp


def oracle_runs(cfg, inp, nb_iter=NIT):
    segs = panda_segs()
    return [oracle_solve_instance(cfg, inp, i, nb_iter, True, segs) for i in range(len(inp["q0"]))]


def binding(runs):
    """(n, per-row counts): the instances whose oracle AL solve stays finite and bounded (|x| < 1e3), and for every row the number of them
    that end with lambda > 0 somewhere on the horizon."""
    ok = [r for r in runs if np.isfinite(r["cost"]) and np.all(np.isfinite(r["X"])) and np.all(np.abs(r["X"]) < 1e3) and np.all(np.isfinite(r["lam"]))]
    m = runs[0]["lam"].shape[1]
    return len(ok), np.array([sum(bool(np.any(r["lam"][:, j] > 0)) for r in ok) for j in range(m)], dtype=int)


def binds(runs):
    """The condition every case must meet ON THE ORACLE's own AL solve: at least three quarters of the rows end with lambda > 0 somewhere on the
    horizon for at least 2 and at most n - 2 of the n finite and bounded instances, and n >= B // 2.  Returns (met, n, counts)."""
    n, cnt = binding(runs)
    good = int(np.sum((cnt >= 2) & (cnt <= n - 2)))
    return (n >= len(runs) // 2 and 4 * good >= 3 * len(cnt)), n, cnt


def multipliers_reference(lam_prev, X, U, A, b, pen):
    """max(0, lambda + pen (A [x_k; u_k] - b_k)) for k = 0 .. T-2 in numpy.longdouble: AL-ILQR.cpp:202-208 restated.  pen is the penalty in
    force at the update, already scaled (the update that closes iteration `it` uses penalty * scaling ** ((it + 1) // lag))."""
    return np.maximum(pp.multiplier_update(lam_prev, X, U, A, b, pen)[0], 0)


def lam_tolerance(cfg, inp, nb_iter=NIT):
    """How far the multipliers of an instance on the oracle's path may be from the oracle's after the solve: every update adds pen a_r . z, and
    check_case lets z differ by X_TOL / U_TOL per entry -- the sum over the updates of pen * sum_j |a_rj| tol_j.  [T-1 or 1][m]"""
    A = np.asarray(inp["A"], float)
    n_u = inp["U0"].shape[2]
    tol_z = np.r_[np.full(A.shape[-1] - n_u, X_TOL), np.full(n_u, U_TOL)]
    pens = sum(pp.al_penalty(cfg["al"], u) for u in range(1, nb_iter // cfg["al"]["lag"] + 1))
    return pens * (np.abs(A) @ tol_z).reshape(-1, A.shape[-2])


def check_case(ctx, cfg, desc, inp, tag, nb_iter=NIT):
    """horizons.check_case (the parity proof with the multiplier check, gains at every step, trajectories) plus the multipliers after the
    solve against the oracle's for the instances on the oracle's path (those check_case compares trajectories of)."""
    got = {}
    line = hz.check_case(ctx, cfg, desc, inp, tag, nb_iter=nb_iter, out=got)
    lam, cost, iters, at = got["lam"], got["cost"], got["iters"], got["alpha"]
    runs = [got["runs"][i] for i in range(len(inp["q0"]))]  # the oracle's own solves of the batch
    met, n_ok, cnt = binds(runs)
    assert met, f"{tag}: the rows do not bind on the oracle's solve ({n_ok} finite instances, per-row counts {cnt.tolist()}): the case tests nothing"
    tol = lam_tolerance(cfg, inp, nb_iter)
    n = 0
    for i, r in enumerate(runs):
        same = int(iters[i]) == r["iters"] and np.array_equal(at[i][: r["iters"]], r["trace_alpha"])
        if not (same and np.isfinite(r["cost"]) and np.isfinite(cost[i]) and np.all(np.abs(r["X"]) < 1e3)):
            continue
        if abs(cost[i] - r["cost"]) > 1e-7 * max(abs(r["cost"]), 1e-12):
            continue
        dev = np.abs(lam[i] - r["lam"])
        assert np.all(dev <= tol), f"{tag}: multipliers of instance {i} are {dev.max():.3e} from the oracle's (step, row {np.argwhere(dev > tol)[0]}; allowed {tol.max():.3e})"
        n += 1
    return f"{line}; multipliers of {n} against the oracle's"


def host_cases():
    """The cases of tests/tools/hostsim/al_shape_checks.py (the host build of the generic kernels, through the C ABI)."""
    out = []
    for name in ("C3", "C2ndal", "C4t1al", "C4al", "C1jal", "C1tal"):
        out += [_case(name, "v1", m, layout) for m in (4, 16, 17, 32) for layout in ("state", "dense")]
        out += [_case(name, "v1", 5, "control"), _case(name, "v1", 16, per_step=True)]
    return out + [_case("C3", "v1", 4, T=T) for T in RESIDUE_HORIZONS]
