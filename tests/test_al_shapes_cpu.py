"""AL-iLQR at every constraint-row capacity, without a GPU (tests/al_shapes.py).

test_rows_bind: the condition that keeps the device matrix of tests/test_gpu_al_shapes.py from being vacuous, asserted on the ORACLE's own AL
solve of every case of it -- at least three quarters of the rows end with lambda > 0 somewhere on the horizon for at least 2 and at most n - 2
of the n instances that stay finite and bounded, n >= B // 2.  Pairs the residue test leaves out because the condition cannot hold there
(al_shapes.RESIDUE_DROPPED): C2ndal and C4al at T = 2, where the one step a row can bind on is k = 0 and every velocity is zero there.

test_al_shapes_on_host_build: the generic kernels and the C-ABI orchestration built with g++ (as tests/test_horizons_cpu.py builds them), driven
by tests/tools/hostsim/al_shape_checks.py in a child process of its own: m in {4, 16, 17, 32} on every AL system shape, control rows, one set
per step, the ring horizons, and set_constraints / reset_multipliers / get_lambda with more than one row."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import al_shapes as al
from tests.helpers import OracleFK, build_hostsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTSIM = os.path.join(ROOT, "tests", "tools", "hostsim")


@pytest.mark.parametrize("test", al.TESTS)
def test_rows_bind(test):
    ctx, seen = OracleFK(), set()
    for c in al.cases(test):
        key = (c["name"], c["R"], c["m"], c["layout"], c["per_step"], c["T"])  # (the pin does not reach the oracle)
        if key in seen:
            continue
        seen.add(key)
        cfg, desc, inp = al.make(ctx, c)
        assert cfg["al"]["lag"] == al.LAG and not np.any(inp["lambda0"]) and inp["lambda0"].shape == (al.B, c["T"] - 1, c["m"])
        assert inp["A"].shape == ((c["T"] - 1,) if c["per_step"] else ()) + (c["m"], inp["A"].shape[-1])
        met, n, cnt = al.binds(al.oracle_runs(cfg, inp))
        assert met, f"{al.case_id(c)}: {n} finite instances, instances with lambda > 0 per row {cnt.tolist()}"


def test_residue_horizons_dropped():
    """What the residue test leaves out is what is written down, and nothing else is missing from 2 .. 14."""
    got = {(c["name"], c["T"]) for c in al.cases("rows_at_ring_residues")}
    assert got == {(n, T) for n in ("C3", "C2ndal", "C4al") for T in range(2, 15)} - {("C2ndal", 2), ("C4al", 2)}


def test_row_layouts():
    rng = np.random.default_rng(0)
    A = al.make_rows(8, 8, 17, "state", rng)
    assert np.all(np.count_nonzero(A, axis=1) == 1) and not np.any(A[:, 8:])
    assert A[7, 7] == 1 and A[8, 0] == -1 and A[15, 7] == -1 and A[16, 0] == 1  # the time state; the sign flips on every wrap
    D = al.make_rows(7, 7, 4, "dense", rng)
    assert np.count_nonzero(D, axis=1).tolist() == [1, 7, 1, 1] and not np.any(D[:, 7:])
    Cn = al.make_rows(8, 8, 5, "control", rng)
    assert Cn[0, 8] == 1 and Cn[1, 15] == -1 and np.count_nonzero(Cn[:2]) == 2 and Cn[2, 2] == 1


def test_multipliers_reference_is_the_plain_update():
    rng = np.random.default_rng(1)
    T, nx, nu, m = 6, 3, 2, 4
    X, U, lam = rng.standard_normal((T, nx)), rng.standard_normal((T - 1, nu)), np.abs(rng.standard_normal((T - 1, m)))
    A, b = rng.standard_normal((T - 1, m, nx + nu)), rng.standard_normal((T - 1, m))
    want = np.array([[max(0.0, lam[k, r] + 0.3 * (A[k, r] @ np.r_[X[k], U[k]] - b[k, r])) for r in range(m)] for k in range(T - 1)])
    np.testing.assert_allclose(np.asarray(al.multipliers_reference(lam, X, U, A, b, 0.3), float), want, rtol=0, atol=1e-14)
    np.testing.assert_allclose(np.asarray(al.multipliers_reference(lam, X, U, A[0], b[0], 0.3), float)[0], want[0], rtol=0, atol=1e-14)


def test_al_shapes_on_host_build(tmp_path):
    lib = build_hostsim(tmp_path / "libilqr_hostsim.so")
    r = subprocess.run([sys.executable, os.path.join(HOSTSIM, "al_shape_checks.py"), lib], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1] == "al shapes: ok"
