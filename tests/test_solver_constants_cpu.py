"""The Riccati solvers away from the default reg, alpha_floor and stop_tol, without a GPU (tests/solver_constants.py).

test_default_constants_are_the_literals: the oracle's test aid orc_set_constants leaves the default path alone -- a solve of C2, C3, C2nd and C4
with the constants never set, and one with (1e-6, 1e-3, 1e-3) set explicitly, agree bit for bit in X, U, K, d, both traces and the multipliers.
test_constants_reach_the_oracle_and_are_restored: a constant changes what the oracle computes, and only inside its solve or block.
test_probe_holds_the_longest_schedule, test_n_alpha_of, test_make_writes_the_descriptor: the plumbing around the table.
test_cases_bite: the conditions that keep the device table of tests/test_gpu_solver_constants.py from being vacuous (solver_constants.bite), on
the ORACLE's own solves of every (workload, horizon, constant set) of it.
test_table: the table is what the module says it is.
test_proof_reads_the_constants: parity_proof.decisions_follow takes the floor of the case, and keeps 1e-3 for the batch solvers.
test_solver_constants_on_host_build: the [v1] cases end to end on the host build of the generic kernels (as tests/test_horizons_cpu.py builds
them), driven by tests/tools/hostsim/solver_constants_checks.py in a child process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import parity_proof as pp
from tests import solver_constants as sc
from tests.helpers import OracleFK, build_hostsim, oracle_solve_instance, orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")
FIELDS = ("X", "fX", "U", "K", "d", "trace_cost", "trace_alpha")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("name", ("C2", "C3", "C2nd", "C4"))
def test_default_constants_are_the_literals(name):
    from tests import horizons as hz

    cfg, desc, inp = hz.make_case(OracleFK(), name, 14)
    explicit = dict(cfg, constants=dict(reg=1e-6, alpha_floor=1e-3, stop_tol=1e-3))
    for i in range(4):
        a, b = oracle_solve_instance(cfg, inp, i, sc.NIT, True), oracle_solve_instance(explicit, inp, i, sc.NIT, True)
        assert a["iters"] == b["iters"] and _bits(a["cost"]) == _bits(b["cost"])
        for f in FIELDS + (("lam",) if cfg["solver"] == "al" else ()):
            assert np.array_equal(_bits(a[f]), _bits(b[f])), f"{name} instance {i}: {f}"


def test_constants_reach_the_oracle_and_are_restored():
    from tests import horizons as hz

    cfg, desc, inp = hz.make_case(OracleFK(), "C2", 14)
    base = oracle_solve_instance(cfg, inp, 0, 1, False)
    r = oracle_solve_instance(dict(cfg, constants=dict(reg=1e-2)), inp, 0, 1, False)
    assert not np.allclose(r["K"], base["K"], rtol=1e-3, atol=0)
    again = oracle_solve_instance(cfg, inp, 0, 1, False)
    assert np.array_equal(_bits(again["K"]), _bits(base["K"])), "the constants outlived their solve"
    with orc.constants(alpha_floor=0.3):  # the context manager: in force inside, the literals after -- also when the block raises
        inside = oracle_solve_instance(cfg, inp, 0, 1, False)
    assert np.array_equal(_bits(inside["K"]), _bits(base["K"]))
    with pytest.raises(ZeroDivisionError):
        with orc.constants(reg=1.0):
            1 / 0
    assert np.array_equal(_bits(oracle_solve_instance(cfg, inp, 0, 1, False)["K"]), _bits(base["K"]))
    with pytest.raises(AssertionError):
        orc.full_constants(dict(regularisation=1.0))


def test_probe_holds_the_longest_schedule():
    """The probe holds more than the 16 step sizes it was built for (ORC_MAX_TRIALS = 64, the cap of n_alpha_of): the 21 of the table's lowest
    floor are all recorded."""
    from tests import horizons as hz

    cfg, desc, inp = hz.make_case(OracleFK(), "C1j", 14)
    cfg["constants"] = dict(alpha_floor=1e-6)
    states = [dict(U=inp["U0"], X=None, lam=None)]
    pr = pp.one_step(cfg, inp, 0, 0, states)["probe"][0]
    assert len(pr["alpha"]) == 21 == sc.n_alpha_of(1e-6) and pr["alpha"][-1] == 2.0 ** -20


def test_n_alpha_of():
    assert [sc.n_alpha_of(f) for f in (0.125, 0.1, 1e-3, 4e-5, 2e-5, 1e-6, 1e-300)] == [4, 5, 11, 16, 17, 21, 64]


def test_table():
    cs = sc.cases()
    assert len(cs) == len({sc.case_id(c) for c in cs}) == 7 * 15 + 1 + 3 * 10
    assert {c["set"] for c in cs} == set(sc.SETS)
    for c in cs:  # which side of the plan's change at n_alpha = 16 a case is on
        n = sc.n_alpha_of(sc.SETS[c["set"]].get("alpha_floor", 1e-3))
        assert (n > 16) == (c["set"] in sc.PAST16_SETS), sc.case_id(c)
    assert set(sc.OVERRIDES) <= {(c["name"], c["set"]) for c in cs}
    assert [sc.case_id(c) for c in sc.host_cases() if c["set"] == "reg-0"] == ["C2-v1-T25-reg-0", "C4t1-v1-T26-reg-0"]


def test_make_writes_the_descriptor():
    ctx = OracleFK()
    for cset, want in (("combined", (1e-2, 2e-5, 1e-1)), ("reg-0", (0.0, 1e-3, 1e-3)), ("floor-2^-3", (1e-6, 0.125, 1e-3))):
        cfg, desc, inp = sc.make(ctx, dict(name="C2", pin="default", set=cset, T=25))
        assert (desc.reg, desc.alpha_floor, desc.stop_tol) == want
        assert tuple(pp.constants_of(cfg)[k] for k in ("reg", "alpha_floor", "stop_tol")) == want


def test_proof_reads_the_constants():
    pr = dict(cost0=1.0, alpha=[1.0, 0.5, 0.25, 0.125, 0.0625], cost=[2.0, 2.0, 2.0, 2.0, 0.5])
    assert pp.decisions_follow(pr, 0.125, alpha_floor=0.125)[0]           # the floor is a step size: the search ends ON it
    assert not pp.decisions_follow(pr, 0.0625, alpha_floor=0.125)[0]      # ... and not one below
    assert pp.decisions_follow(pr, 0.0625, alpha_floor=0.1)[0]            # 0.125 > 0.1 goes on
    assert pp.decisions_follow(pr, 0.0625)[0] and not pp.decisions_follow(pr, 0.125)[0]  # absent: the reference's 1e-3
    assert not pp.decisions_follow(pr, 0.125, floor_strict=True, alpha_floor=0.125)[0]  # the batch solvers keep 1e-3
    assert pp.constants_of(dict()) == dict(reg=1e-6, alpha_floor=1e-3, stop_tol=1e-3)
    assert pp.constants_of(dict(constants=dict(stop_tol=0.1))) == dict(reg=1e-6, alpha_floor=1e-3, stop_tol=0.1)


@pytest.mark.parametrize("cset", list(sc.SETS))
def test_cases_bite(cset):
    ctx = OracleFK()
    for c in sc.oracle_cases():
        if c["set"] != cset:
            continue
        cfg, desc, inp = sc.make(ctx, c)
        met, facts = sc.bite(c, cfg, inp)
        print(sc.case_id(c), facts)
        assert met, f"{sc.case_id(c)}: {facts}"


def test_solver_constants_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "solver_constants_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "solver constants: ok"
