"""Multi-start solves (ilqr_problem_adopt, ilqr_problem_spread_controls, ilqr_problem_select, ilqr_problem_get_at) -- cases and checks shared by
tests/tools/hostsim/multistart_checks.py (the host build of the generic kernels) and tests/test_gpu_multistart.py (the device kernels).

Systems: C3 (PosOrn-1 with one AL row: solve_al), C4 (PosOrnTime-2), chain3 (a 3-joint chain: the mapped layouts) at T = 2, 3, 9.  Groups
(G, S): (13, 1), (5, 3), (1, 70) everywhere -- an odd remainder of Bp and an S that crosses a wave -- and (3, 64), (2, 65), (128, 16) on the device;
at B = 2048 select, get_at and adopt run on plans that were solved as two halves on two streams (SPLIT_CASES).

(a) select   exactly a NumPy restatement on the caller's scores (ties, -0 / +0, +-inf, NaN, a group with nobody eligible, a group whose only
             finite member is not eligible); score = NULL is get_cost; an instance made NONFINITE by a NaN control never wins.
(b) get_at   the indexed rows of the full getters, == on bytes; repeated and descending indices; the host form refuses -1 and B, the _dev form clamps.
(c) adopt    after adopt(all bits that apply) a solve on dst gives the bytes of a fresh problem fed through the host setters with the gathered
             arrays (0 and 3 iterations); every bit alone; invalidation; every refusal by its text; src unmoved.
(d) spread   U0 (read through a 0-iteration solve's get_U) = base + sigma z with z of tests/closed_loop_noise.normals at the stated counters, within
             that module's draw bound plus one ulp of the sum; member 0 and sigma-0 entries on bytes; a cut-out with offsets on bytes.
(e) pipeline a planted winner (member 2 starts from the converged controls of its task, the others from zeros) wins every group after one
             coarse iteration, and the refined result is, byte for byte, a direct solve from those controls.
Every _dev form takes its arrays through an `arrays` object: HostArrays here (on the host build a device pointer is a host pointer), torch tensors
in the device test."""
from __future__ import annotations

import numpy as np

from ilqr_planner_amd import capi, workloads
from tests import closed_loop as cl
from tests import closed_loop_noise as cn
from tests import gains as gn
from tests import narrow_chain as nc

SYSTEMS = ("C3", "C4", "chain3")
HORIZONS = (2, 3, 9)
GROUPS = ((13, 1), (5, 3), (1, 70))
GROUPS_DEVICE = ((3, 64), (2, 65))
BIG = (128, 16)        # B = 2048, the smallest batch with split halves
# The plans that are solved as two halves on two streams at that size (ilqr_plan.hpp: plan_riccati): C4 under AUTO (the wave-per-instance MFMA
# sweep, any solve of at least one iteration), and C3 only under ilqr_ctx_set_split(2) (AUTO keeps the single-integrator pipeline on one stream)
# (tests/cpp/plan_table_main.cpp holds the rule: c4(2048) splits, c4(2049) takes the rows sweep and does not)
SPLIT_CASES = (("C4", None), ("C3", 2))   # (system, set_split mode or None for the default)
NIT = 3
ALL_BITS = capi.ADOPT_STATE | capi.ADOPT_TARGETS | capi.ADOPT_CONTROLS | capi.ADOPT_MULTIPLIERS
BAD_STATUS = capi.STATUS_NONFINITE | capi.STATUS_SWEEP_IO


class HostArrays:
    """The arrays of a _dev call on the host build: a device pointer is a host pointer."""

    def put(self, a):
        return np.ascontiguousarray(a).copy()

    def empty(self, shape, dtype=np.float64):
        return np.zeros(shape, dtype=dtype)

    def ptr(self, h):
        return h.ctypes.data

    def get(self, h):
        return h


def make_case(ctx, name, T, B, seed=None):
    """(cfg, desc, inp) of a system at horizon T and batch B; C3 carries its AL row (inp A, b, lambda0)."""
    if name == "chain3":
        cfg = dict(nc.narrow_cfg("C2", 3), T=T)
        desc, inp = workloads.make_batch(ctx, cfg, B=B, chain=nc.capi_chain(3), seed=seed)
        return cfg, desc, inp
    cfg = dict(workloads.config(name), T=T)
    if name in cl.TIME_SHAPES:   # the batch seeds of tests/closed_loop.py: the plans stay bounded
        desc, inp = workloads.make_batch(ctx, cfg, B=B, seed=seed if seed is not None else cl.TIME_PLANS.get((name, T), (1, 0))[0])
        inp["U0"][:, :, -1] = np.sqrt(cfg["ctimes"][-1] / (T - 1))
    else:
        desc, inp = workloads.make_batch(ctx, cfg, B=B, seed=seed)
    if cfg.get("al"):   # an update inside NIT iterations: the multipliers of a plan differ from lambda0 and between instances
        cfg["al"] = dict(cfg["al"], lag=2)
    return cfg, desc, inp


def is_al(cfg):
    return bool(cfg.get("al"))


def take(inp, idx):
    """The inputs of the instances idx."""
    out = dict(inp, q0=inp["q0"][idx], dq0=inp["dq0"][idx], targets=[t[idx] for t in inp["targets"]], U0=inp["U0"][idx])
    if "lambda0" in inp:
        out["lambda0"] = inp["lambda0"][idx]
    return out


def solve(p, cfg, n, penalty=None):
    if is_al(cfg):
        al = cfg["al"]
        p.solve_al(n, al["lag"], al["penalty"] if penalty is None else penalty, al["scaling"], True, False)
    else:
        p.solve_recursive(n, True, False)


def results(p, cfg):
    r = dict(X=p.X(), U=p.U(), cost=p.cost(), K=p.K(), d=p.d(), iters=p.iters(), status=p.status())
    if is_al(cfg):
        r["lam"] = p.lam()
    return r


def same(a, b, tag):
    for k, v in a.items():
        assert v.tobytes() == b[k].tobytes(), f"{tag}: {k} differs ({int(np.sum(v != b[k]))} entries, NaN counted)"


def final_penalty(nb_iter, lag, penalty, scaling):
    """The penalty an AL solve of nb_iter iterations ends with: one multiplication per update iteration (ilqr_capi_solve.cpp: solve_riccati)."""
    for it in range(nb_iter):
        if (it + 1) % lag == 0:
            penalty *= scaling
    return penalty


# ------------------------------------------------------------------------------------------------ (a) select

def select_ref(score, eligible, status, S):
    """The definition of include/ilqr_hip.h, restated."""
    B = len(score)
    G = B // S
    win, best, n = np.empty(G, np.int32), np.empty(G), np.empty(G, np.int32)
    for g in range(G):
        cand = [b for b in range(g * S, (g + 1) * S) if (eligible is None or eligible[b] != 0) and not (status[b] & BAD_STATUS) and np.isfinite(score[b])]
        n[g] = len(cand)
        if cand:
            w = min(cand, key=lambda b: (float(score[b]), b))   # float compare: -0.0 == 0.0, the tie goes to the lower b
            win[g], best[g] = w, score[w]
        else:
            win[g], best[g] = g * S, np.nan
    return win, best, n


def same_selection(got, ref, tag):
    assert np.array_equal(got.winner, ref[0]), f"{tag}: winner {got.winner} against {ref[0]}"
    assert np.array_equal(got.n_candidates, ref[2]), f"{tag}: n_candidates {got.n_candidates} against {ref[2]}"
    assert np.array_equal(np.isnan(got.best), np.isnan(ref[1])), f"{tag}: best {got.best} against {ref[1]}"
    ok = ~np.isnan(ref[1])
    assert got.best[ok].tobytes() == ref[1][ok].tobytes(), f"{tag}: best {got.best} against {ref[1]} (signs of zero included)"


def scores(G, S, rnd, rng):
    """Scores and flags of round rnd: few distinct values (ties), both zeros, +-inf and NaN; round 1: nobody in group 0 is eligible;
    round 2: the last group's only finite member is not eligible; round 3: no flags."""
    B = G * S
    vals = np.array([-2.0, -0.0, 0.0, 0.5, 0.5, 1.0, 3.0, np.inf, -np.inf, np.nan])
    score = vals[rng.integers(0, len(vals), B)]
    score[rng.integers(0, B)] = -0.0
    elig = (rng.random(B) < 0.7).astype(np.int32) * rng.integers(1, 5, B).astype(np.int32)   # any non-zero value counts
    if rnd == 1:
        elig[:S] = 0
    if rnd == 2:
        g = G - 1
        score[g * S:(g + 1) * S] = vals[rng.integers(7, 10, S)]
        score[g * S + S // 2] = -1.0
        elig[g * S + S // 2] = 0
    return score, (None if rnd == 3 else elig)


def select_dev(p, arrays, S, score, elig):
    G = p.B // S
    hs = arrays.put(score) if score is not None else None
    he = arrays.put(elig.astype(np.int32)) if elig is not None else None
    hw, hb, hn = arrays.empty(G, np.int32), arrays.empty(G), arrays.empty(G, np.int32)
    p.select_dev(S, arrays.ptr(hs) if hs is not None else None, arrays.ptr(he) if he is not None else None, arrays.ptr(hw), arrays.ptr(hb), arrays.ptr(hn))
    p.ctx.synchronize()
    return capi.Selection(np.array(arrays.get(hw)), np.array(arrays.get(hb)), np.array(arrays.get(hn)))


def check_select(ctx, arrays, name, T, G, S, tag):
    B = G * S
    cfg, desc, inp = make_case(ctx, name, T, B)
    p = workloads.load_batch(ctx, desc, inp, B)
    rng = np.random.default_rng(1000 * G + S)
    try:
        cl._refused(lambda: p.select(S), "ilqr_problem_select needs a plan")
        U0 = inp["U0"].copy()
        bad = (G // 2) * S + min(1, S - 1)   # an instance whose rollout is not finite; no first member: a group without a candidate names that one
        U0[bad, 0, 0] = np.nan
        p.set_controls(U0)
        solve(p, cfg, 1)
        status, cost = p.status(), p.cost()
        assert status[bad] & capi.STATUS_NONFINITE and np.sum(status & capi.STATUS_NONFINITE) == 1, f"{tag}: status {status}"
        same_selection(p.select(S), select_ref(cost, None, status, S), f"{tag} score=NULL")
        same_selection(select_dev(p, arrays, S, None, None), select_ref(cost, None, status, S), f"{tag} score=NULL _dev")
        for rnd in range(4):
            score, elig = scores(G, S, rnd, rng)
            score[bad] = -100.0           # the best score of its group, and it must not win
            if elig is not None:
                elig[bad] = 1
            ref = select_ref(score, elig, status, S)
            assert not np.any(ref[0] == bad) or S == 1
            got = p.select(S, score, elig)
            same_selection(got, ref, f"{tag} round {rnd}")
            assert np.all(got.winner != bad) or S == 1, f"{tag}: the NONFINITE instance won"
            if S == 1:
                assert got.n_candidates[bad] == 0 and got.winner[bad] == bad and np.isnan(got.best[bad])
            same_selection(select_dev(p, arrays, S, score, elig), ref, f"{tag} round {rnd} _dev")
            only = p.select(S, score, elig, want_best=False, want_n_candidates=False)
            assert np.array_equal(only.winner, ref[0]) and only.best is None
        cl._refused(lambda: p.select(S, want_winner=False, want_best=False, want_n_candidates=False), "are all null pointers")
        cl._refused(lambda: p.select(0), "group_size must be >= 1")
        if B > 1:
            cl._refused(lambda: p.select(B + 1), "is not a multiple of group_size")
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (b) get_at

def check_get_at(ctx, arrays, name, T, B, tag):
    cfg, desc, inp = make_case(ctx, name, T, B)
    p = workloads.load_batch(ctx, desc, inp, B)
    try:
        solve(p, cfg, NIT)
        full = dict(X=p.X(), U=p.U(), cost=p.cost(), iters=p.iters(), status=p.status())
        rng = np.random.default_rng(B)
        for idx in (np.arange(B)[::-1], np.array([B - 1, 0, 0, B // 2, B // 2, B - 1, 0]), rng.integers(0, B, 2 * B + 3), np.array([B // 3])):
            r = p.get_at(idx)
            for k, v in full.items():
                assert getattr(r, k).tobytes() == v[idx].tobytes(), f"{tag}: get_at {k} differs from the full getter's rows"
            r = p.get_at(idx, want_X=False, want_iters=False)
            assert r.X is None and r.iters is None and r.U.tobytes() == full["U"][idx].tobytes() and r.status.tobytes() == full["status"][idx].tobytes()
        cl._refused(lambda: p.get_at([0, -1]), "index[1] = -1 is outside 0 .. %d" % (B - 1))
        cl._refused(lambda: p.get_at([B]), "index[0] = %d is outside 0 .. %d" % (B, B - 1))
        cl._refused(lambda: p.get_at([0], False, False, False, False, False), "every output is a null pointer")
        cl._refused(lambda: p.get_at(np.zeros(0, np.int32)), "n must be >= 1")
        # the _dev form clamps
        idx = np.array([-5, 0, B - 1, B, B + 70, -1, B // 2], dtype=np.int32)
        cidx = np.clip(idx, 0, B - 1)
        n = len(idx)
        hi = arrays.put(idx)
        hX, hU, hc = arrays.empty((n, T, p.dims.n_x)), arrays.empty((n, T - 1, p.dims.n_u)), arrays.empty(n)
        hit, hst = arrays.empty(n, np.int32), arrays.empty(n, np.int32)
        p.get_at_dev(n, arrays.ptr(hi), arrays.ptr(hX), arrays.ptr(hU), arrays.ptr(hc), arrays.ptr(hit), arrays.ptr(hst))
        ctx.synchronize()
        for k, h in (("X", hX), ("U", hU), ("cost", hc), ("iters", hit), ("status", hst)):
            assert np.array(arrays.get(h)).tobytes() == full[k][cidx].tobytes(), f"{tag}: get_at_dev {k} differs from the clamped rows"
    finally:
        p.close()


# ------------------------------------------------------------------------------------------------ (c) adopt

def load(ctx, desc, inp, B, lam=None):
    """workloads.load_batch with the multipliers `lam` where given."""
    return workloads.load_batch(ctx, desc, dict(inp, lambda0=lam) if lam is not None else inp, B)


def check_adopt(ctx, arrays, name, T, B_dst, B_src, tag, dev_form=False):
    """The whole of (c) for one pair of batch sizes; dev_form: adopt through ilqr_problem_adopt_dev."""
    cfg, desc, inp_s = make_case(ctx, name, T, B_src)
    _, _, inp_d = make_case(ctx, name, T, B_dst, seed=77)    # dst's own inputs: another draw
    al = is_al(cfg)
    rng = np.random.default_rng(B_dst + 31 * B_src)
    idx = rng.integers(0, B_src, B_dst).astype(np.int32)
    idx[0], idx[-1] = B_src - 1, 0
    src = workloads.load_batch(ctx, desc, inp_s, B_src)
    made = [src]

    def adopt(dst, what):
        if dev_form:
            h = arrays.put(idx)
            dst.adopt_dev(src, arrays.ptr(h), what)
            ctx.synchronize()
        else:
            dst.adopt(src, idx, what)

    try:
        solve(src, cfg, NIT)
        src.gains()   # alpha all ones, as tests/gains.check_unmoved wants it; the plan and the multipliers stay (tests/gains.py (c))
        before, gains_before = gn.snapshot(src, NIT), dict(K=src.K(), d=src.d())
        Us, lam_s = before["U"], before.get("lam")
        bits = ALL_BITS if al else ALL_BITS & ~capi.ADOPT_MULTIPLIERS
        for n in (0, NIT):
            # all bits that apply, into a problem that was given nothing but its rows
            dst = capi.BatchProblem(ctx, desc, B_dst)
            made.append(dst)
            if al:
                dst.set_constraints(inp_d["A"], inp_d["b"], None)
            adopt(dst, bits)
            cl._refused(dst.gains, "ilqr_problem_gains needs a plan")
            solve(dst, cfg, n)
            got = results(dst, cfg)
            dst.gains()   # accepted again after a solve
            ref = load(ctx, desc, dict(take(inp_s, idx), U0=Us[idx]), B_dst, lam_s[idx] if al else None)
            made.append(ref)
            solve(ref, cfg, n)
            same(got, results(ref, cfg), f"{tag} all bits, {n} iterations")
        # CONTROLS0: the controls src was given
        dst = capi.BatchProblem(ctx, desc, B_dst)
        made.append(dst)
        if al:
            dst.set_constraints(inp_d["A"], inp_d["b"], inp_d["lambda0"])
        adopt(dst, capi.ADOPT_STATE | capi.ADOPT_TARGETS | capi.ADOPT_CONTROLS0)
        solve(dst, cfg, 1)
        ref = load(ctx, desc, dict(take(inp_s, idx), lambda0=inp_d.get("lambda0")), B_dst)
        made.append(ref)
        solve(ref, cfg, 1)
        same(results(dst, cfg), results(ref, cfg), f"{tag} STATE | TARGETS | CONTROLS0")
        # every bit alone, into a problem that holds inputs (and a plan) of its own
        g = take(inp_s, idx)
        alone = [(capi.ADOPT_STATE, dict(q0=g["q0"], dq0=g["dq0"]), None), (capi.ADOPT_TARGETS, dict(targets=g["targets"]), None),
                 (capi.ADOPT_CONTROLS0, dict(U0=g["U0"]), None), (capi.ADOPT_CONTROLS, dict(U0=Us[idx]), None)]
        if al:
            alone.append((capi.ADOPT_MULTIPLIERS, {}, lam_s[idx]))
        for bit, change, lam in alone:
            dst = workloads.load_batch(ctx, desc, inp_d, B_dst)
            made.append(dst)
            solve(dst, cfg, 1)
            dst.gains()
            lam_now = dst.lam() if al else None
            adopt(dst, bit)
            cl._refused(dst.gains, "ilqr_problem_gains needs a plan")
            cl._refused(lambda: dst.closed_loop(samples=1), "closed loop needs the gains")
            solve(dst, cfg, 1)
            ref = load(ctx, desc, dict(inp_d, **change), B_dst, lam if lam is not None else lam_now)
            made.append(ref)
            solve(ref, cfg, 1)
            same(results(dst, cfg), results(ref, cfg), f"{tag} bit {bit} alone")
        gn.check_unmoved(before, gn.snapshot(src, NIT), src.alpha(), f"{tag}: src")
        same(gains_before, dict(K=src.K(), d=src.d()), f"{tag}: src moved")
    finally:
        for p in made:
            p.close()


def check_adopt_refusals(ctx, tag):
    cfg, desc, inp = make_case(ctx, "C3", 9, 5)
    cfg4, desc4, inp4 = make_case(ctx, "C4", 9, 5)
    _, desc_T, _ = make_case(ctx, "C3", 3, 5)
    _, desc_c, inp_c = make_case(ctx, "chain3", 9, 5)
    ctx2 = capi.Context(0)
    made = []
    try:
        src = workloads.load_batch(ctx, desc, inp, 5)
        dst = workloads.load_batch(ctx, desc, inp, 5)
        other = workloads.load_batch(ctx2, desc, inp, 5)
        made += [src, dst, other]
        idx = np.arange(5, dtype=np.int32)
        R = cl._refused
        R(lambda: dst.adopt(src, idx, capi.ADOPT_CONTROLS), "ILQR_ADOPT_CONTROLS needs a plan in src")
        solve(src, cfg, 1)
        R(lambda: dst.adopt(other, idx, capi.ADOPT_STATE), "both problems must belong to one context")
        R(lambda: dst.adopt(dst, idx, capi.ADOPT_STATE), "dst and src are the same problem")
        for d_, field in ((desc4, "kind"), (desc_T, "horizon"), (desc_c, "dof")):
            q = capi.BatchProblem(ctx, d_, 5)
            made.append(q)
            R(lambda: q.adopt(src, idx, capi.ADOPT_STATE), f"the problems differ in {field}")
        d2 = capi.ProblemDesc.from_buffer_copy(bytes(desc4))
        d2.nb_deriv = 1   # PosOrnTime-1 against PosOrnTime-2
        q4, q41 = workloads.load_batch(ctx, desc4, inp4, 5), capi.BatchProblem(ctx, d2, 5)
        made += [q4, q41]
        R(lambda: q41.adopt(q4, idx, capi.ADOPT_STATE), "the problems differ in nb_deriv")
        d3 = capi.ProblemDesc.from_buffer_copy(bytes(desc))
        d3.n_kp = 1
        q1 = capi.BatchProblem(ctx, d3, 5)
        made.append(q1)
        R(lambda: q1.adopt(src, idx, capi.ADOPT_STATE), "the problems differ in n_kp")
        d5 = capi.ProblemDesc.from_buffer_copy(bytes(desc))
        d5.kp_joint[0] = 1   # the via point as a joint-space keypoint: its target rows are a state, not f(x)
        qj = capi.BatchProblem(ctx, d5, 5)
        made.append(qj)
        R(lambda: qj.adopt(src, idx, capi.ADOPT_TARGETS), "ILQR_ADOPT_TARGETS needs equal kp_joint flags (keypoint 0")
        qj.adopt(src, idx, capi.ADOPT_STATE | capi.ADOPT_CONTROLS0)   # the other bits do not look at it
        R(lambda: dst.adopt(src, idx, 0), "`what` must be a combination of the ILQR_ADOPT_* bits")
        R(lambda: dst.adopt(src, idx, 32), "`what` must be a combination of the ILQR_ADOPT_* bits")
        R(lambda: dst.adopt(src, idx, capi.ADOPT_CONTROLS0 | capi.ADOPT_CONTROLS), "both name dst's U0")
        empty = capi.BatchProblem(ctx, desc, 5)
        made.append(empty)
        R(lambda: dst.adopt(empty, idx, capi.ADOPT_STATE), "ILQR_ADOPT_STATE needs a start state in src")
        R(lambda: dst.adopt(empty, idx, capi.ADOPT_CONTROLS0), "ILQR_ADOPT_CONTROLS0 needs controls in src")
        R(lambda: dst.adopt(empty, idx, capi.ADOPT_MULTIPLIERS), "ILQR_ADOPT_MULTIPLIERS needs constraint rows in both problems")
        A2 = np.vstack([inp["A"], inp["A"]])
        empty.set_constraints(A2, np.array([2.0, 2.5]), None)
        R(lambda: dst.adopt(empty, idx, capi.ADOPT_MULTIPLIERS), "ILQR_ADOPT_MULTIPLIERS needs rows of equal m and per_step")
        bad = idx.copy()
        bad[3] = 5
        R(lambda: dst.adopt(src, bad, capi.ADOPT_STATE), "index[3] = 5 is outside 0 .. 4")
        bad[3] = -1
        R(lambda: dst.adopt(src, bad, capi.ADOPT_STATE), "index[3] = -1 is outside 0 .. 4")
        assert dst.L.ilqr_problem_adopt(dst.h, src.h, None, capi.ADOPT_STATE) != 0 and b"index is a null pointer" in dst.L.ilqr_last_error(ctx.h)
        assert dst.L.ilqr_problem_adopt(dst.h, None, idx.ctypes.data, capi.ADOPT_STATE) != 0 and b"src is a null pointer" in dst.L.ilqr_last_error(ctx.h)
    finally:
        for p in made:
            p.close()
        ctx2.close()


def check_adopt_dev_clamps(ctx, arrays, tag):
    """The _dev form with indices outside src's batch: the clamped rows."""
    cfg, desc, inp = make_case(ctx, "chain3", 3, 5)
    src = workloads.load_batch(ctx, desc, inp, 5)
    dst = capi.BatchProblem(ctx, desc, 7)
    idx = np.array([-3, 0, 4, 5, 1 << 30, -(1 << 31), 2], dtype=np.int32)
    c = np.clip(idx, 0, 4)
    ref = workloads.load_batch(ctx, desc, take(inp, c), 7)
    try:
        h = arrays.put(idx)
        dst.adopt_dev(src, arrays.ptr(h), capi.ADOPT_STATE | capi.ADOPT_TARGETS | capi.ADOPT_CONTROLS0)
        solve(dst, cfg, 1)
        solve(ref, cfg, 1)
        same(results(dst, cfg), results(ref, cfg), f"{tag}: adopt_dev with clamped indices")
    finally:
        for p in (src, dst, ref):
            p.close()


# ------------------------------------------------------------------------------------------------ (d) spread

def sigma_u(nu, scale=1e-2):
    """As tests/closed_loop_noise.sigma_vectors: every entry drawn but entry 1 (a half-used pair) and, from n_u = 6, the pair (4, 5) (not generated)."""
    s = scale * (1.0 - 0.03125 * np.arange(nu))
    if nu > 1:
        s[1] = 0.0
    if nu >= 6:
        s[4:6] = 0.0
    return s


def normals_u(seed, G, S, T1, nu, group_offset=0, member_offset=0):
    """z[G][S][T-1][n_u] of the counters (group_offset + g, member_offset + s, k, j)."""
    return cn.draw(seed, G, S, range(T1), nu, group_offset, member_offset)


def read_u0(p, cfg):
    solve(p, cfg, 0)
    return p.U()


def check_spread(ctx, name, T, G, S, tag):
    B = G * S
    cfg, desc, inp = make_case(ctx, name, T, B)
    rng = np.random.default_rng(5 * G + S)
    nu = inp["U0"].shape[2]
    base = inp["U0"] + 0.05 * rng.standard_normal(inp["U0"].shape)
    sig = sigma_u(nu)
    seed, go, mo = 0x1234567887654321, 7, 0
    p = workloads.load_batch(ctx, desc, dict(inp, U0=base), B)
    made = [p]
    try:
        assert read_u0(p, cfg).tobytes() == base.tobytes()
        p.gains()
        p.spread_controls(S, seed, sig, go, mo)
        cl._refused(p.gains, "ilqr_problem_gains needs a plan")
        U = read_u0(p, cfg)
        z = normals_u(seed, G, S, T - 1, nu, go, mo).reshape(B, T - 1, nu)
        member = np.arange(B) % S
        exp = base + np.where((member != 0)[:, None, None], sig * z, 0.0)
        bound = cn._draw_bound(sig, z) + np.spacing(np.abs(exp))
        dev = np.abs(U - exp)
        assert np.all(dev <= bound), f"{tag}: U0 is not base + sigma z: {np.max(dev / np.maximum(bound, 1e-300)):.3g} bounds"
        assert U[member == 0].tobytes() == base[member == 0].tobytes(), f"{tag}: member 0 moved"
        assert U[..., sig == 0.0].tobytes() == base[..., sig == 0.0].tobytes(), f"{tag}: an entry with sigma 0 moved"
        if S > 1:
            moved = U[member != 0][..., sig != 0.0] != base[member != 0][..., sig != 0.0]
            assert np.mean(moved) > 0.99, f"{tag}: the other members did not move"
        # a scalar sigma draws every entry; with member_offset > 0 member 0 of the call is not the global member 0 and moves too
        p.set_controls(base)
        p.spread_controls_dev(S, seed, 1e-2, go, 3)
        U2 = read_u0(p, cfg)
        z2 = normals_u(seed, G, S, T - 1, nu, go, 3).reshape(B, T - 1, nu)
        exp2 = base + 1e-2 * z2
        assert np.all(np.abs(U2 - exp2) <= cn._draw_bound(1e-2, z2) + np.spacing(np.abs(exp2))), f"{tag}: member_offset 3"
        # a cut-out of groups and members, run with its offsets, is the large call's bytes
        g0, g1 = (G // 3, G // 3 + max(1, G // 2)) if G > 1 else (0, 1)
        s0, s1 = (S // 3, S // 3 + max(1, S // 2)) if S > 1 else (0, 1)
        rows = np.array([g * S + s for g in range(g0, g1) for s in range(s0, s1)])
        q = workloads.load_batch(ctx, desc, dict(take(inp, rows), U0=base[rows]), len(rows))
        made.append(q)
        q.spread_controls(s1 - s0, seed, sig, go + g0, mo + s0)
        assert read_u0(q, cfg).tobytes() == U[rows].tobytes(), f"{tag}: the cut-out differs from the large call"
        # refusals
        R = cl._refused
        R(lambda: p.spread_controls(0, seed, sig), "group_size must be >= 1")
        R(lambda: p.spread_controls(B + 1, seed, sig), "is not a multiple of group_size")
        neg = sig.copy()
        neg[-1] = -1e-3
        R(lambda: p.spread_controls(S, seed, neg), "every sigma_u must be finite and >= 0")
        neg[-1] = np.inf
        R(lambda: p.spread_controls(S, seed, neg), "every sigma_u must be finite and >= 0")
        neg[-1] = np.nan
        R(lambda: p.spread_controls(S, seed, neg), "every sigma_u must be finite and >= 0")
        if G > 1:   # (with one group the first offset out of range is 2^32 itself: no unsigned int)
            R(lambda: p.spread_controls(S, seed, sig, group_offset=2 ** 32 - G + 1), "exceeds 2^32")
        if S > 1:
            R(lambda: p.spread_controls(S, seed, sig, member_offset=2 ** 32 - S + 1), "exceeds 2^32")
        p.spread_controls(S, seed, sig, group_offset=2 ** 32 - G, member_offset=2 ** 32 - S)   # the last counters are in range
        e = capi.BatchProblem(ctx, desc, B)
        made.append(e)
        R(lambda: e.spread_controls(S, seed, sig), "ilqr_problem_spread_controls needs controls")
    finally:
        for x in made:
            x.close()


# ------------------------------------------------------------------------------------------------ (e) pipeline

PIPELINE = ("C3", "chain3")   # the systems of the planted-winner check (T = 9): an AL solve and a plain one
NCONV = 12      # iterations of the earlier solve whose controls are planted
NREFINE = 4


def planted(ctx, name, T, G):
    """(cfg, desc, inp, Uconv): the tasks and the controls an earlier solve of each converged to."""
    cfg, desc, inp = make_case(ctx, name, T, G)
    p = workloads.load_batch(ctx, desc, inp, G)
    try:
        solve(p, cfg, NCONV)
        Uconv = p.U()
    finally:
        p.close()
    return cfg, desc, inp, Uconv


def check_planted_condition(name, cfg, inp, Uconv, tag):
    """The condition on the input, judged by the oracle: after one iteration the converged start's cost is below the zero start's."""
    from tests.helpers import oracle_solve_instance

    if name == "chain3":
        segs = nc.oracle_segs(3)
        one = lambda i_, g: nc.oracle_solve(cfg, i_, g, segs, 1, False)   # noqa: E731
    else:
        one = lambda i_, g: oracle_solve_instance(cfg, i_, g, 1, False)   # noqa: E731
    for g in range(len(Uconv)):
        c_zero = one(inp, g)["cost"]
        c_conv = one(dict(inp, U0=Uconv), g)["cost"]
        assert c_conv < c_zero, f"{tag}: task {g} is no planted-winner case for the oracle ({c_conv} against {c_zero})"


def check_pipeline(ctx, arrays, cfg, desc, inp, Uconv, S, tag, member=2):
    G = len(Uconv)
    B = G * S
    al = is_al(cfg)
    rep = (np.arange(B) // S).astype(np.int32)
    U0 = np.repeat(inp["U0"], S, axis=0)
    U0[member::S] = Uconv
    tasks = workloads.load_batch(ctx, desc, inp, G)
    starts = capi.BatchProblem(ctx, desc, B)
    direct = load(ctx, desc, dict(inp, U0=Uconv), G)
    made = [tasks, starts, direct]
    try:
        if al:
            starts.set_constraints(inp["A"], inp["b"], np.repeat(inp["lambda0"], S, axis=0))
        h = arrays.put(rep)
        starts.adopt_dev(tasks, arrays.ptr(h), capi.ADOPT_STATE | capi.ADOPT_TARGETS)
        starts.set_controls(U0)
        solve(starts, cfg, 1)
        hw = arrays.empty(G, np.int32)
        starts.select_dev(S, None, None, arrays.ptr(hw), None, None)
        ctx.synchronize()
        win = np.array(arrays.get(hw))
        assert np.array_equal(win, np.arange(G) * S + member), f"{tag}: winners {win}, costs {starts.cost().reshape(G, S)}"
        tasks.adopt_dev(starts, arrays.ptr(hw), capi.ADOPT_CONTROLS | (capi.ADOPT_MULTIPLIERS if al else 0))
        pen = final_penalty(1, cfg["al"]["lag"], cfg["al"]["penalty"], cfg["al"]["scaling"]) if al else None
        solve(tasks, cfg, NREFINE, pen)
        got = results(tasks, cfg)
        # the direct solve: one iteration from the planted controls, then continued from its own plan
        solve(direct, cfg, 1)
        cont = load(ctx, desc, dict(inp, U0=direct.U()), G, direct.lam() if al else None)
        made.append(cont)
        solve(cont, cfg, NREFINE, pen)
        same(got, results(cont, cfg), f"{tag}: refined against direct")
    finally:
        for p in made:
            p.close()


# ------------------------------------------------------------------------------------------------ (f) the sequence of solveMultiStart, by hand

def multistart_by_hand(ctx, cfg, desc, inp, S, seed, sigma, coarse_iter, nb_iter):
    """Steps 1 to 7 of solveMultiStart through capi.BatchProblem: (results of the G tasks, Selection, coarse_first)."""
    G = len(inp["q0"])
    B = G * S
    al = is_al(cfg)
    tasks = workloads.load_batch(ctx, desc, inp, G)
    starts = capi.BatchProblem(ctx, desc, B)
    try:
        if al:
            starts.set_constraints(inp["A"], inp["b"], np.repeat(inp["lambda0"], S, axis=0))
        starts.adopt(tasks, np.arange(B) // S, capi.ADOPT_STATE | capi.ADOPT_TARGETS | capi.ADOPT_CONTROLS0)
        starts.spread_controls(S, seed, sigma)
        solve(starts, cfg, coarse_iter)
        sel = starts.select(S)
        first = starts.get_at(np.arange(G) * S, want_X=False, want_U=False, want_iters=False, want_status=False).cost
        tasks.adopt(starts, sel.winner, capi.ADOPT_CONTROLS | (capi.ADOPT_MULTIPLIERS if al else 0))
        solve(tasks, cfg, nb_iter, final_penalty(coarse_iter, cfg["al"]["lag"], cfg["al"]["penalty"], cfg["al"]["scaling"]) if al else None)
        r = dict(X=tasks.X(), U=tasks.U(), cost=tasks.cost(), alpha=tasks.alpha(), iters=tasks.iters(), status=tasks.status())
        return r, sel, first
    finally:
        tasks.close()
        starts.close()


def continued_by_hand(ctx, cfg, desc, inp, coarse_iter, nb_iter):
    """A solve of coarse_iter iterations, continued from its own plan through adopt(CONTROLS [| MULTIPLIERS]) for nb_iter more."""
    G = len(inp["q0"])
    al = is_al(cfg)
    a, b = workloads.load_batch(ctx, desc, inp, G), workloads.load_batch(ctx, desc, inp, G)
    try:
        solve(a, cfg, coarse_iter)
        b.adopt(a, np.arange(G), capi.ADOPT_CONTROLS | (capi.ADOPT_MULTIPLIERS if al else 0))
        solve(b, cfg, nb_iter, final_penalty(coarse_iter, cfg["al"]["lag"], cfg["al"]["penalty"], cfg["al"]["scaling"]) if al else None)
        return dict(X=b.X(), U=b.U(), cost=b.cost(), alpha=b.alpha(), iters=b.iters(), status=b.status())
    finally:
        a.close()
        b.close()
