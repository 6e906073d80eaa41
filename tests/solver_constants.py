"""The Riccati solvers away from the default reg, alpha_floor and stop_tol -- shared by tests/test_gpu_solver_constants.py (the device kernels),
tests/test_solver_constants_cpu.py (the oracle-only conditions) and tests/tools/hostsim/solver_constants_checks.py (the host build of the generic
kernels).

ilqr_problem_desc carries three constants a caller may set.  The oracle restates the reference, where they are literals; its test aid
orc_set_constants (oracle/ilqr_oracle.h) replaces them in the Riccati solvers, and a case carries them as cfg["constants"], which
helpers.oracle_solve_instance and tests/parity_proof.py read -- make() writes the same values into the descriptor.  What a constant set reaches
(csrc/ilqr_plan.hpp: n_alpha_of, plan_riccati):

  floor-2^-3   alpha_floor = 0.125: n_alpha = 4, and the floor IS a step size (`alpha > floor` against `>=`); NA = 11 templates with 4 live rows
  floor-0.1    n_alpha = 5 (the last step size 0.0625 is below the floor); the speculated step size of k_forward_mfma clamped to n_alpha - 1
  floor-4e-5   n_alpha = 16: the NA = 16 instantiations of every cooperative forward pass
  floor-2e-5   n_alpha = 17, the first count past them: the generic forward pass under the cooperative sweeps, k_backward_si_dpp<FUSED = false>
               (plain records, Is through the ring), Init::Lti + k_al_post for AL
  floor-1e-6   n_alpha = 21, the case tests/cpp/plan_table_main.cpp checks the plan of
  reg-1e-2     the regularisation enters the inverse only (quirk D-3): at 1e-2 a sweep that put it into the value update, or dropped one of its
  reg-0        terms, moves the gains far beyond their tolerance; at 0 the reg terms of the closed forms vanish
  stop-1e-1    stops early / never stops: the three spellings of the stop rule beside the literal cost < 1e-3 of the non-AL rule
  stop-1e-9
  combined     floor 2e-5, reg 1e-2, stop 1e-1

Every case is gated by horizons.check_case, unchanged: the parity proof with instances 0 and 1 always proven, gains at every step after 1 and NIT
iterations, trajectories where the path is the oracle's, every multiplier update for AL.  Every (workload, set) pair must BITE -- bite() below, asserted
on the oracle alone by tests/test_solver_constants_cpu.py for the whole table."""
from __future__ import annotations

import numpy as np

from tests import al_shapes as al
from tests import horizons as hz
from tests import parity_proof as pp
from tests.helpers import oracle_solve_instance, panda_segs

B = hz.B   # 13: ragged on every path
NIT = 6

SETS = {
    "floor-2^-3": dict(alpha_floor=0.125),
    "floor-0.1": dict(alpha_floor=0.1),
    "floor-4e-5": dict(alpha_floor=4e-5),
    "floor-2e-5": dict(alpha_floor=2e-5),
    "floor-1e-6": dict(alpha_floor=1e-6),
    "reg-1e-2": dict(reg=1e-2),
    "reg-0": dict(reg=0.0),
    "stop-1e-1": dict(stop_tol=1e-1),
    "stop-1e-9": dict(stop_tol=1e-9),
    "combined": dict(alpha_floor=2e-5, reg=1e-2, stop_tol=1e-1),
}
COOPERATIVE_SETS = ("floor-2^-3", "floor-0.1", "floor-4e-5", "reg-1e-2", "reg-0", "stop-1e-1", "stop-1e-9")  # n_alpha <= 16
PAST16_SETS = ("floor-2e-5", "floor-1e-6", "combined")                                                      # n_alpha > 16

# horizon per workload: T - 1 = 13 and 25 are odd and leave non-zero residues in the rings of depth 3, 4 and 8; T = 26 has T - 2 = 24, the full ring
HORIZON = {"C2": 25, "C2r": 14, "C3": 26, "C3rows4": 25, "C1j": 14, "C2nd": 25, "C4t1": 26, "C4": 14, "C4al": 25}

COOPERATIVE = [("C2", "dpp"), ("C2", "wg"), ("C2r", "dpp"), ("C3", "dpp"), ("C3", "wg"), ("C1j", "default"), ("C2nd", "mfma"), ("C2nd", "rows"),
               ("C4t1", "mfma-dpp"), ("C4t1", "rows-rows"), ("C4", "mfma-dpp"), ("C4", "rows-rows"), ("C4al", "default"), ("C2", "v1"), ("C4t1", "v1")]
# "C3rows4": C3 with the binding 4-row state-only set of tests/al_shapes.py (MR = 4 in the non-fused sweep)
PAST16 = [("C2", "default"), ("C2r", "default"), ("C3", "default"), ("C1j", "default"), ("C3rows4", "default"), ("C2nd", "mfma"), ("C2nd", "rows"),
          ("C4t1", "mfma-dpp"), ("C4t1", "rows-rows"), ("C4al", "default")]
EXTRA_PINS = {"wglds": dict(ILQR_HIP_PATH="v2", ILQR_FWD="wglds")}  # k_forward_wg, the predecessor of k_forward_reg (not in test_gpu_horizons.PINS)


def _case(name, pin, cset):
    return dict(name=name, pin=pin, set=cset, T=HORIZON[name])


def case_id(c):
    return f"{c['name']}-{c['pin']}-T{c['T']}-{c['set']}"


def cases():
    """The device table of tests/test_gpu_solver_constants.py."""
    out = [_case(n, p, s) for s in COOPERATIVE_SETS for n, p in COOPERATIVE]
    out.append(_case("C3", "wglds", "floor-4e-5"))
    out += [_case(n, p, s) for s in PAST16_SETS for n, p in PAST16]
    return out


def host_cases():
    """The [v1] cases: the generic kernels, also run on their host build (tests/tools/hostsim/solver_constants_checks.py)."""
    return [c for c in cases() if c["pin"] == "v1"]


def oracle_cases():
    """One case per (workload, horizon, constant set): the pin does not reach the oracle."""
    seen, out = set(), []
    for c in cases():
        key = (c["name"], c["T"], c["set"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


# ----------------------------------------------------------------------------- inputs
#
# Input overrides, (workload, constant set) -> tuple of dicts: where the stock batch of workloads.make_batch (horizons.make_case) misses a condition
# of bite(), the inputs are shaped until the ORACLE's solve meets it (tests/test_solver_constants_cpu.py holds every case to it).  Each dict shapes
# the instances i with i % who[0] == who[1] (a condition asks for instances on both sides of a decision; the others keep the stock inputs):
#   u0      their initial joint controls are drawn from U(-u0, u0) (seeded) in place of zero: a poor start, whose sweeps propose steps the line
#           search has to cut
#   far     their keypoint positions (joint systems: joint targets) are scaled by this factor: out of reach, or far enough for the control cost at
#           the keypoint steps to stay above the 1e-3 of the non-AL stop rule -- the solve runs all its iterations
#   near    their keypoint targets are the poses (joint systems: the joint angles) of configurations within `near` of the start: they converge
#           within the first iterations, reach cost < 1e-3 and the early-stop thresholds one after the other, and then sit where no step size improves
#           (not closer than that where the precisions weigh the orientation: the angle of a pose error comes from an arc cosine near 1, so a
#           cost carries an absolute error of about 1e-16, and the proof compares costs to 1e-9 relative -- near = 0.1 keeps them above 1e-6)
#   spread  ... each of them closer than the one before by this factor, so that their first steps are spread over the decades between two thresholds
#   at_goal their keypoint targets are the start's own pose: cost 0 from the first rollout on, no step size improves on it, the line search runs to
#           the floor at once (with reg = 1e-2 the regularised step of every other instance descends at full length, iteration after iteration)
#   lam0    their AL multipliers start at this value in place of the bound (the tutorial's start, which alone drives a first step of full size)
#   warm    their initial controls are the oracle's own after `warm` iterations with the default constants and no early stop -- a warm start close
#           to the iteration's fixed point.  There the sweep's direction is dominated by the control-cost gradient R u of the steps WITHOUT a
#           keypoint, which the measured cost does not contain (quirk D-2): about every other line search finds no step size that improves and runs
#           to the floor, by margins far above rounding (targets within 1e-7 of the start do the same with costs of 1e-19, where the cost of a
#           state is itself only good to 1e-8 and the proof's tolerances have nothing to hold on to)
#   dt0     their time control starts at this value in place of the duration the last keypoint asks for (horizons.make_case)
_ODD, _EVEN = (2, 1), (2, 0)
OVERRIDES = {
    # --- raised floors: the stock batch ends a line search at the floor on at most one instance (C2, C2r), or on all but one (C3, C1j, C2nd, C4,
    # C4al: with a floor of 1/8 the accept-anyway rule takes steps that send the time systems to costs that are not finite)
    ("C2", "floor-2^-3"): (dict(far=1.5, who=_ODD),),  # out-of-reach goals: 4 instances end at the floor
    ("C2r", "floor-2^-3"): (dict(far=1.5, who=_ODD),),
    ("C3", "floor-2^-3"): (dict(lam0=0.0, who=_EVEN),),  # without the multipliers' push the even instances never reach the floor
    ("C1j", "floor-2^-3"): (dict(u0=0.1, at_goal=True, who=_EVEN),),  # an LQ problem sits at the floor from its second step on; the even ones start at their goal and stop at once
    ("C2nd", "floor-2^-3"): (dict(u0=0.5, who=_ODD), dict(u0=0.1, who=_EVEN)),
    ("C4", "floor-2^-3"): (dict(at_goal=True, who=_EVEN),),  # the even instances improve with a full first step and stop: never at the floor, and finite
    ("C4al", "floor-2^-3"): (dict(near=0.02, lam0=0.0, who=(1, 0)), dict(dt0=0.05, who=(3, 0))),  # a tame batch, every third with a short step
    ("C2", "floor-0.1"): (dict(far=1.5, who=_ODD),),
    ("C2r", "floor-0.1"): (dict(far=1.5, who=_ODD),),
    ("C1j", "floor-0.1"): (dict(u0=0.1, at_goal=True, who=_EVEN),),
    ("C2nd", "floor-0.1"): (dict(u0=0.5, who=_ODD),),
    ("C4", "floor-0.1"): (dict(at_goal=True, who=_EVEN),),
    ("C4al", "floor-0.1"): (dict(at_goal=True, lam0=0.0, who=_EVEN),),
    # --- floors below 1e-3: no instance of the stock batch of the PosOrn-1 and time-1 systems rejects eleven step sizes within 6 iterations; the even
    # instances converge within them and then sit where no step size improves
    ("C2", "floor-4e-5"): (dict(near=0.02, who=_EVEN),),
    ("C2r", "floor-4e-5"): (dict(near=0.02, who=_EVEN),),
    ("C3", "floor-4e-5"): (dict(near=0.1, who=_EVEN),),
    ("C4t1", "floor-4e-5"): (dict(near=0.1, who=_EVEN),),
    ("C2", "floor-2e-5"): (dict(near=0.02, who=_EVEN),),
    ("C2r", "floor-2e-5"): (dict(near=0.02, who=_EVEN),),
    ("C3", "floor-2e-5"): (dict(near=0.1, who=_EVEN),),
    ("C3rows4", "floor-2e-5"): (dict(near=0.1, who=_EVEN),),
    ("C4t1", "floor-2e-5"): (dict(near=0.1, who=_EVEN),),
    ("C2", "floor-1e-6"): (dict(near=0.02, who=_EVEN),),
    ("C2r", "floor-1e-6"): (dict(near=0.02, who=_EVEN),),
    ("C3", "floor-1e-6"): (dict(near=0.1, who=_EVEN),),
    ("C3rows4", "floor-1e-6"): (dict(near=0.1, who=_EVEN),),
    ("C4t1", "floor-1e-6"): (dict(near=0.1, who=_EVEN),),
    # --- stop_tol: no instance of the stock batch stops within 6 iterations under any of the three thresholds (the non-AL rule also wants
    # cost < 1e-3), C1j stops after 2 under 1e-3 and 1e-1 alike, C4al after 1 or 2 under 1e-1.  The shaped instances pass 1e-1 and 1e-3 in
    # different iterations and never 1e-9; the others run all 6
    ("C2", "stop-1e-1"): (dict(near=0.1, who=_EVEN),),
    ("C2r", "stop-1e-1"): (dict(warm=10, who=_EVEN),),  # warm-started instances pass the two thresholds in different iterations
    ("C3", "stop-1e-1"): (dict(near=0.02, who=_ODD),),
    ("C1j", "stop-1e-1"): (dict(far=1.5, who=_ODD), dict(near=0.0001, who=_EVEN)),  # far: the control cost stays above 1e-3
    ("C2nd", "stop-1e-1"): (dict(near=0.02, who=_ODD), dict(near=0.3, who=_EVEN)),
    ("C4t1", "stop-1e-1"): (dict(near=0.3, who=_EVEN),),
    ("C4", "stop-1e-1"): (dict(near=0.3, who=_EVEN),),
    ("C4al", "stop-1e-1"): (dict(u0=0.1, who=_EVEN),),  # a poor start keeps three instances going for all 6
    ("C2", "stop-1e-9"): (dict(near=0.02, who=_EVEN),),
    ("C2r", "stop-1e-9"): (dict(near=0.02, who=_EVEN),),
    ("C3", "stop-1e-9"): (dict(near=0.1, who=_EVEN),),
    ("C2nd", "stop-1e-9"): (dict(near=0.1, who=_EVEN),),
    ("C4t1", "stop-1e-9"): (dict(at_goal=True, who=_EVEN),),
    ("C4", "stop-1e-9"): (dict(at_goal=True, who=_EVEN),),
    # --- combined: with reg = 1e-2 the regularised step descends at full length iteration after iteration, so a step size below 2^-10 is accepted
    # only where the sweep's direction is not the measured cost's, or where no step moves the cost at all
    ("C2", "combined"): (dict(near=0.3, warm=3, who=_EVEN),),  # warm-started next to the fixed point
    ("C2r", "combined"): (dict(near=0.3, warm=3, who=_EVEN),),
    ("C3rows4", "combined"): (dict(lam0=2.0, who=_EVEN),),  # multipliers above zero on slack rows, as the stock C3 starts: the sweep's direction is not the cost's
    ("C1j", "combined"): (dict(at_goal=True, who=_EVEN),),  # at the goal, exactly (joint space)
    ("C2nd", "combined"): (dict(near=0.1, who=_EVEN),),
    ("C4t1", "combined"): (dict(dt0=0.0, who=(6, 3)), dict(near=0.02, who=_EVEN)),  # two start with the time control at zero: B = 0, no step moves the cost
    ("C4al", "combined"): (dict(lam0=0.0, who=_EVEN),),
}


def _override(name, cset):
    return OVERRIDES.get((name, cset), ())


def _shape(ctx, cfg, desc, inp, ov):
    """Applies one override dict to the inputs in place."""
    Bn, T = inp["U0"].shape[0], cfg["T"]
    mod, res = ov.get("who", (1, 0))
    who = np.arange(Bn) % mod == res
    rng = np.random.default_rng(77)
    tm = 1 if cfg.get("ctimes") else 0
    nj = inp["U0"].shape[2] - tm
    joint = cfg["kind"] in (2, 3)
    if "dt0" in ov:
        assert tm, "dt0: time systems only"
        inp["U0"][who, :, -1] = ov["dt0"]
    if ov.get("u0"):
        inp["U0"][who, :, :nj] = rng.uniform(-ov["u0"], ov["u0"], (Bn, T - 1, nj))[who]
    if ov.get("far"):
        for t in inp["targets"]:
            t[who, 0:(nj if joint else 3)] *= ov["far"]
    if ov.get("near") or ov.get("at_goal"):
        for k, t in enumerate(inp["targets"]):
            dist = (0.0 if ov.get("at_goal") else ov["near"]) / float(ov.get("spread", 1.0)) ** np.cumsum(who)  # (spread: from instance to instance)
            q = inp["q0"] + dist[:, None] * rng.uniform(-1.0, 1.0, inp["q0"].shape)
            if tm:  # ... reached at the time the initial controls take to the keypoint's step
                t[who, -1] = inp["kp_t"][k] * inp["U0"][who, 0, -1] ** 2
            if joint:
                t[who, :nj] = q[who, :nj]
            else:
                pos, quat, _ = ctx.fk_batch(desc, q)
                t[who, 0:3], t[who, 3:7] = pos[who], quat[who]
    if ov.get("warm"):
        plain = {k: v for k, v in cfg.items() if k != "constants"}
        trial = dict(inp, U0=inp["U0"].copy())
        for i in np.flatnonzero(who):
            inp["U0"][i] = oracle_solve_instance(plain, trial, i, ov["warm"], False, panda_segs())["U"]
    if "lam0" in ov:
        inp["lambda0"][who] = ov["lam0"]


def make(ctx, c, override=None):
    """(cfg, desc, inp) of a case: cfg["constants"] holds the set, the descriptor's three fields the same values.  override: in place of the table's."""
    name, T, cset = c["name"], c["T"], c["set"]
    if name == "C3rows4":
        cfg, desc, inp = al.make_case(ctx, "C3", T, 4, "state", nb_iter=NIT)
    else:
        cfg, desc, inp = hz.make_case(ctx, name, T)
    ov = _override(name, cset) if override is None else override
    for o in ov:
        _shape(ctx, cfg, desc, inp, o)
    consts = dict(SETS[cset])
    cfg["constants"] = consts
    for k, v in consts.items():
        setattr(desc, k, float(v))
    return cfg, desc, inp


def check_case(ctx, cfg, desc, inp, tag):
    """horizons.check_case as it stands, then the status words: bit ILQR_STATUS_ALPHA_FLOOR (2) is set exactly where the instance's last line search
    ended at or below the case's floor (`<=`: with a floor of 2^-3 the floor is itself a step size), bit NONFINITE (1) exactly where the cost is
    not finite."""
    got = {}
    line = hz.check_case(ctx, cfg, desc, inp, tag, nb_iter=NIT, out=got)
    floor = pp.constants_of(cfg)["alpha_floor"]
    n_floor = 0
    for i, (st, n) in enumerate(zip(got["status"], got["iters"])):
        assert n >= 1, f"{tag}: instance {i} made no iteration"
        last = got["alpha"][i, int(n) - 1]
        assert bool(st & 2) == bool(last <= floor), f"{tag}: status {st} of instance {i}, whose last line search ended at {last} (floor {floor})"
        assert bool(st & 1) == (not np.isfinite(got["cost"][i])), f"{tag}: status {st} of instance {i}, cost {got['cost'][i]}"
        n_floor += bool(st & 2)
    return f"{line}; {n_floor} end at the floor"


# ----------------------------------------------------------------------------- the conditions every case must meet on the oracle alone

GAIN_RTOL, GAIN_ATOL = 1e-6, 1e-7  # horizons._check_gains on K


def oracle_runs(cfg, inp, nb_iter=NIT, constants="case"):
    """The oracle's solves of the batch with early stop; constants: "case" = the case's, None = the reference's literals."""
    segs = panda_segs()
    cf = cfg if constants == "case" else {k: v for k, v in cfg.items() if k != "constants"}
    return [oracle_solve_instance(cf, inp, i, nb_iter, True, segs) for i in range(len(inp["q0"]))]


def n_alpha_of(alpha_floor):
    """csrc/ilqr_plan.hpp n_alpha_of with a line search, restated."""
    a, n = 1.0, 1
    while a > alpha_floor and n < 64:
        a *= 0.5
        n += 1
    return n


def bite(c, cfg, inp):
    """(met, facts): the conditions of a case's constant set on the oracle's own solves.
      floors below 1e-3   at least 2 instances accept a step size below 2^-10 in some iteration
      raised floors       at least 2 instances end a line search at the floor (the last step size of the schedule), at least 2 never do
      reg                 K after one iteration differs from the default-constants K by more than 100 x the gain tolerance somewhere, on
                          each of the always-proven instances 0 and 1
      stop_tol            at least 2 instances run another number of iterations than under the defaults; for 1e-1 at least 2 run all NIT
      all                 the cost is finite on a majority of instances"""
    consts = SETS[c["set"]]
    runs = oracle_runs(cfg, inp)
    n = len(runs)
    facts = dict(finite=sum(bool(np.isfinite(r["cost"])) for r in runs))
    met = 2 * facts["finite"] > n
    if "alpha_floor" in consts:
        fl = consts["alpha_floor"]
        if fl < 1e-3:
            facts["below_2^-10"] = sum(bool(np.any(r["trace_alpha"] < 2.0 ** -10)) for r in runs)
            met = met and facts["below_2^-10"] >= 2
        else:
            last = 0.5 ** (n_alpha_of(fl) - 1)
            facts["at_floor"] = sum(bool(np.any(r["trace_alpha"] == last)) for r in runs)
            facts["never_at_floor"] = n - facts["at_floor"]
            assert all(np.all(r["trace_alpha"] >= last) for r in runs)
            met = met and facts["at_floor"] >= 2 and facts["never_at_floor"] >= 2
    if "reg" in consts:
        r1, r0 = oracle_runs(cfg, inp, 1), oracle_runs(cfg, inp, 1, constants=None)
        ratio = [float(np.max(np.abs(a["K"] - b["K"]) / (GAIN_ATOL + GAIN_RTOL * np.abs(b["K"])))) for a, b in zip(r1, r0)]
        facts["K_moves_by_tolerances"] = [round(x, 1) for x in ratio[:2]]
        met = met and all(x > 100 for x in ratio[:2])
    if "stop_tol" in consts:
        r0 = oracle_runs(cfg, inp, NIT, constants=None)
        facts["other_iters"] = sum(a["iters"] != b["iters"] for a, b in zip(runs, r0))
        facts["iters"] = [r["iters"] for r in runs]
        met = met and facts["other_iters"] >= 2
        if consts["stop_tol"] == 1e-1:
            met = met and sum(r["iters"] == NIT for r in runs) >= 2
    return met, facts
