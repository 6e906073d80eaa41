"""Riccati solves at short and odd horizons against the oracle -- shared by tests/test_gpu_horizons.py (the device kernels) and
tests/tools/hostsim/horizon_checks.py (the host build of the generic kernels and the C-ABI orchestration).

Every pipelined kernel of the Riccati path walks the horizon through a prefetch ring of fixed depth (3, 4 or 8 steps): the horizons
T = 2 .. 25 reach every residue of T - 1 and T - 2 modulo lcm(3, 4, 8) = 24 and every horizon shorter than a ring.  A mistake in a
ring's tail is wrong only at a few steps near t = 0, so besides the parity proof the gains are compared at every step."""
from __future__ import annotations

import numpy as np

from ilqr_planner_amd import workloads
from tests import parity_proof as pp
from tests.helpers import oracle_solve_instance, orc, panda_segs

HORIZONS = tuple(range(2, 26))
B = 13       # ragged: not a multiple of the 2, 4, 8 or 16 instances a wave holds on any path
NIT = 4      # iterations of the gated solve (early stop on)
KP_HORIZONS = (17, 25)


def kp_placements(T):
    """Keypoint steps that put a keypoint at step 0, two in one 8-step block, and a pair on both sides of a block boundary."""
    return ((0, T - 1), (T - 2, T - 1), (7, 8), (8, 15))


def make_case(ctx, name, T, B=B, kp=None):
    """(cfg, desc, inp) of workload `name` at horizon T; kp: keypoint steps that replace make_batch's (T // 2 - 1, T - 1).
    The time control (dt = u^2) starts at the duration the last keypoint asks for: from make_batch's u = 0.01, a horizon of a dozen steps
    must grow dt a thousandfold, and the first line searches send some instances to costs of 1e21 and beyond, where a NaN on one side only
    is decided by rounding."""
    cfg = dict(workloads.config(name), T=T)
    desc, inp = workloads.make_batch(ctx, cfg, B=B)
    if cfg.get("ctimes"):
        inp["U0"][:, :, -1] = np.sqrt(cfg["ctimes"][-1] / (T - 1))
    if kp is not None:
        assert len(kp) == desc.n_kp and all(0 <= a < b < T for a, b in zip(kp, kp[1:])) and kp[-1] < T
        for k, t in enumerate(kp):
            desc.kp_timestep[k] = int(t)
        inp["kp_t"] = list(kp)
    return cfg, desc, inp


def _same_path(iters, at, r):
    n = r["iters"]
    return int(iters) == n and np.array_equal(at[:n], r["trace_alpha"])


def _check_gains(tag, K, d, iters, at, runs, rerun):
    """K_t, d_t at every step t = 0 .. T-2 of every instance whose oracle run `runs[i]` took its path, at the tolerances of
    test_gains_and_fx_outputs -- or, where the sweep is ill-conditioned (time systems reach cond(Quu) ~ 1e9), within ILL_FACTOR of the
    largest move the oracle's own algebraically neutral variants make (tests/parity_proof.py): rerun(i) repeats runs[i] under the variant
    set.  Returns (instances compared, instances compared by their sensitivity)."""
    n = n_ill = 0
    for i, r in runs.items():
        if not _same_path(iters[i], at[i], r):
            continue
        ill = False
        for name, got, atol in (("K", K[i], 1e-7), ("d", d[i], 1e-9)):
            ref = r[name]
            if np.allclose(got, ref, rtol=1e-6, atol=atol, equal_nan=True):
                continue
            sens = 0.0
            for v in pp.VARIANTS:
                orc.set_variant(v)
                try:
                    rv = rerun(i)
                finally:
                    orc.set_variant(0)
                sens = max(sens, float(np.max(np.abs(rv[name] - ref)))) if _same_path(iters[i], at[i], rv) else np.inf
            dev = float(np.max(np.abs(got - ref)))
            assert dev <= pp.ILL_FACTOR * sens, (f"{tag}: {name} of instance {i} is {dev:.3e} from the oracle's (rtol 1e-6, atol {atol:g} "
                                                 f"exceeded), its own variants move it by {sens:.3e}")
            ill = True
        n += 1
        n_ill += ill
    return n, n_ill


def check_case(ctx, cfg, desc, inp, tag, nb_iter=NIT, always=(0, 1), out=None):
    """One case: a 1-iteration solve (its sweep starts from the same rollout on both sides) and a nb_iter-iteration solve with early stop, both
    against the oracle.  Gates: the parity proof of the longer one (tests/parity_proof.py, instances in `always` proven whatever their
    distance); the gains at every step -- of the 1-iteration solve against the oracle's, of the longer one against the oracle's sweep from
    the device's own state before its last iteration (the iteration that wrote them: a gain image left from an earlier iteration shows
    there, while the drift of an ill-conditioned instance over several iterations does not); the trajectories where the path is the
    oracle's.  Returns a one-line summary; out: a dict that receives the longer solve's cost, iters, step sizes, multipliers (AL), its
    distance to the oracle's runs, those runs and the status words."""
    Bn = len(inp["q0"])
    segs = panda_segs()
    p = workloads.load_batch(ctx, desc, inp, Bn)
    try:
        workloads.run_solver(p, cfg, nb_iter=1, early_stop=True)
        K1, d1, it1, at1 = p.K(), p.d(), p.iters(), p.trace(1)[1]
        runs1 = {i: oracle_solve_instance(cfg, inp, i, 1, True, segs) for i in range(Bn)}
        n1, ill1 = _check_gains(tag + " after 1 iteration", K1, d1, it1, at1, runs1, lambda i: oracle_solve_instance(cfg, inp, i, 1, True, segs))
        assert n1 >= len(always), f"{tag}: only {n1} instance(s) took the oracle's first step"
        if cfg["solver"] == "al":
            p.reset_multipliers()
        workloads.run_solver(p, cfg, nb_iter=nb_iter, early_stop=True)
        K, d, X, U, cost, iters = p.K(), p.d(), p.X(), p.U(), p.cost(), p.iters()
        at = p.trace(nb_iter)[1]
        lam = p.lam() if cfg["solver"] == "al" else None
        status = p.status()
        runs = {}

        def oracle_solve(i):
            runs[i] = oracle_solve_instance(cfg, inp, i, nb_iter, True, segs)
            return runs[i]

        states = []
        summ, rel, failures = pp.check_batch(p, cfg, inp, nb_iter, True, workloads.run_solver, oracle_solve, always=always, states_out=states)
        assert not failures, f"{tag}: {len(failures)} instance(s) neither within 1e-4 nor proven: {failures[:3]}"
        assert summ["frac_unexplained"] == 0.0 and summ["n_proven_always"] == len(always), (tag, summ)
        if len(states) < int(iters.max()):  # (the proof needed fewer re-runs than the gains of the last iteration do)
            states = pp.gpu_states(p, cfg, nb_iter, False, workloads.run_solver, upto=int(iters.max()))
    finally:
        p.close()
    last = {}  # the oracle's iteration from the device's state before each instance's last one, where it takes the device's step size
    for i in range(Bn):
        n = int(iters[i])
        if n > 0:
            r = pp.one_step(cfg, inp, i, n - 1, states, segs, probe=False)
            if r["iters"] == 1 and r["trace_alpha"][0] == at[i, n - 1]:
                last[i] = dict(r, iters=n, trace_alpha=at[i, :n])

    def rerun_last(i):
        r = pp.one_step(cfg, inp, i, int(iters[i]) - 1, states, segs, probe=False)
        return dict(r, iters=int(iters[i]), trace_alpha=np.r_[at[i, :int(iters[i]) - 1], r["trace_alpha"]])

    n4, ill4 = _check_gains(f"{tag} after {nb_iter} iterations", K, d, iters, at, last, rerun_last)
    assert n4 >= len(always), f"{tag}: only {n4} instance(s) took the oracle's step size in their last iteration"
    nxu = 0
    for i, r in runs.items():  # same path: the trajectories agree too (the loose bounds of test_random_batch_vs_oracle: the arm is redundant)
        bounded = np.all(np.abs(r["X"]) < 1e3)  # a diverged AL instance reaches states of 1e76: the proof has checked its every step instead
        if _same_path(iters[i], at[i], r) and rel[i] <= 1e-7 and np.isfinite(r["cost"]) and np.isfinite(cost[i]) and bounded:
            nxo, nuo = r["X"].shape[1], r["U"].shape[1]
            np.testing.assert_allclose(X[i][:, :nxo], r["X"], rtol=0, atol=2e-4, err_msg=f"{tag}: X of instance {i}")
            np.testing.assert_allclose(U[i][:, :nuo], r["U"], rtol=0, atol=2e-3, err_msg=f"{tag}: U of instance {i}")
            nxu += 1
    if out is not None:
        out.update(cost=cost, iters=iters, alpha=at, lam=lam, rel=rel, runs=runs, status=status)
    mult = ""
    if "n_multiplier_checked" in summ:  # AL: every multiplier update recomputed (parity_proof.check_multipliers)
        mult = (f", multipliers of {summ['n_multiplier_checked']} ({summ['n_multiplier_updates']} updates, {summ['n_multiplier_skipped']} skipped, "
                f"{summ['n_clamp_ties']} clamp ties, worst {summ['worst_multiplier_ratio']:.2f} of the bound)")
    return (f"{tag}: gains of {n1} / {n4} instances (1 / {nb_iter} iterations; {ill1} / {ill4} ill-conditioned), trajectories of {nxu}, within 1e-4 "
            f"{summ['frac_within_1e4']:.2f}, proofs {summ['n_proofs']} ({summ['n_steps_checked']} steps, {summ['n_tie_decisions']} ties, "
            f"{summ['n_steps_ill_conditioned']} ill-conditioned, worst step {summ['worst_step_rel']:.1e})" + mult)
