"""The shared tables of the batch Gauss-Newton solvers (sensitivities Wt / Wr, V, H0, G, Et, PZ, ZPZ, the Cholesky inverse), their signature and
the sizes type are plain host C++ (ilqr_planner_amd/csrc/ilqr_batch_tables.hpp).  tests/cpp/batch_tables_main.cpp includes nothing but that header:
without arguments it checks the exact properties, with arguments it writes the tables of one case, which are compared here with a dense restatement
(explicit A, B, dense Su, numpy.linalg for H0^-1)."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, DT = 7, 0.01
R_DIAG = 1e-5 * (1.0 + 0.5 * np.arange(NU))
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("batch_tables") / "batch_tables")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ilqr_planner_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "batch_tables_main.cpp"), "-o", out])
    return out


def test_exact_properties(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok"


def _dense(nd, T, kp_t, psi):
    """Wt at the keypoint steps and the steps before them, the shifted Wr = V, from explicit A, B and dense Su."""
    I, Z = np.eye(NU), np.zeros((NU, NU))
    A = I if nd == 1 else np.block([[I, DT * I], [Z, I]])
    B = DT * I if nd == 1 else np.vstack([DT * DT / 2 * I, DT * I])
    nx, N = nd * NU, (T - 1) * NU

    def su(t, first):  # d x_t / d u: block j is A^(t-1-j) B for first <= j <= t - 1
        S = np.zeros((nx, N))
        for j in range(first, t):
            S[:, j * NU:(j + 1) * NU] = np.linalg.matrix_power(A, t - 1 - j) @ B
        return S

    wt = np.stack([np.stack([su(t, 0) @ psi, su(t - 1, 0) @ psi if t > 0 else np.zeros((nx, psi.shape[1]))]) for t in kp_t])
    wr = np.stack([su(t, 1) @ psi for t in kp_t])  # block 0 of the reference's Su is zero (quirk D-1)
    return wt, wr


def _run(exe, tmp_path, mode, nd, T, kp_t, psi, Kw, ld):
    pf = "-"
    if psi is not None:
        pf = str(tmp_path / "psi.bin")
        np.ascontiguousarray(psi, dtype=np.float64).tofile(pf)
    out = str(tmp_path / "tables.bin")
    subprocess.check_call([exe, mode, str(nd), str(NU), str(T), repr(DT), str(Kw), str(ld), pf, out, str(len(kp_t))] + [str(t) for t in kp_t] +
                          [repr(float(r)) for r in R_DIAG], timeout=60)
    return np.fromfile(out)


def _split(flat, shapes):
    out, o = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(flat[o:o + n].reshape(s))
        o += n
    assert o == flat.size
    return out


CASES = [(nd, T, kp) for nd in (1, 2) for T, kp in ((4, (1, 3)), (12, (1, 11)), (12, (0, 5, 6, 11)))]


def _check(label, names, got, want, n, kappa):
    """Every table within n eps kappa_2(H0) max|table| of the dense restatement: n is the longest chain of sums that feeds a table."""
    for name, g, w in zip(names, got, want):
        bound = n * EPS * kappa * np.abs(w).max()
        ratio = np.abs(g - w).max() / bound if bound > 0 else float(np.abs(g - w).max() > 0)
        print(f"{label} {name}: max err / bound = {ratio:.3e}")
        assert ratio <= 1.0, f"{label}: table {name} is {ratio:.3g} x its bound"


@pytest.mark.parametrize("nd,T,kp_t", CASES, ids=[f"nd{c[0]}-T{c[1]}-kp{'_'.join(map(str, c[2]))}" for c in CASES])
@pytest.mark.parametrize("basis", ["identity", "rbf", "bernstein"])
def test_wide_tables_against_dense(exe, tmp_path, nd, T, kp_t, basis):
    nx, N, nkp = nd * NU, (T - 1) * NU, len(kp_t)
    m = nkp * nx
    psi = np.eye(N) if basis == "identity" else np.kron(orc.psi(basis, T - 1, 3), np.eye(NU))
    Kw = psi.shape[1]
    Rfull = np.tile(R_DIAG, T - 1)
    H0 = psi.T @ (Rfull[:, None] * psi)
    kappa = R_DIAG.max() / R_DIAG.min() if basis == "identity" else np.linalg.cond(H0)
    assert kappa < 1e8
    wt, wr = _dense(nd, T, kp_t, psi)
    V = wr.reshape(m, Kw)
    h0inv = np.linalg.inv(H0)
    Z = h0inv @ V.T
    PZ = psi @ Z
    want = [wt, wr, V @ Z, wt.reshape(2 * m, Kw) @ Z, PZ, PZ.T @ PZ]
    shapes = [wt.shape, wr.shape, (m, m), (2 * m, m), (N, m), (m, m)]
    names = ["Wt", "V", "G", "Et", "PZ", "ZPZ"]
    if basis != "identity":
        want.append(h0inv)
        shapes.append((Kw, Kw))
        names.append("h0inv")
    got = _split(_run(exe, tmp_path, "wide", nd, T, kp_t, None if basis == "identity" else psi, Kw, Kw), shapes)
    _check(f"{basis} nd={nd} T={T} kp={kp_t}", names, got, want, N + Kw + m, kappa)


@pytest.mark.parametrize("nd,T,kp_t", CASES, ids=[f"nd{c[0]}-T{c[1]}-kp{'_'.join(map(str, c[2]))}" for c in CASES])
def test_narrow_tables_against_dense(exe, tmp_path, nd, T, kp_t):
    nx, N, nkp, ld = nd * NU, (T - 1) * NU, len(kp_t), 16
    psi = np.kron(orc.psi("rbf", T - 1, 2), np.eye(NU))
    Kw = psi.shape[1]
    assert Kw == 14
    psip = np.hstack([psi, np.zeros((N, ld - Kw))])
    Rfull = np.tile(R_DIAG, T - 1)
    H0 = psip.T @ (Rfull[:, None] * psip)
    kappa = np.linalg.cond(H0[:Kw, :Kw])
    assert kappa < 1e8
    H0[range(Kw, ld), range(Kw, ld)] = 1.0
    wt, wr = _dense(nd, T, kp_t, psip)
    want = [psip, H0, wt, wr, psip.T @ psip]
    got = _split(_run(exe, tmp_path, "narrow", nd, T, kp_t, psi, Kw, ld), [w.shape for w in want])
    assert np.array_equal(got[0], psip)
    _check(f"narrow nd={nd} T={T} kp={kp_t}", ["psip", "H0", "Wt", "Wr", "pp"], got, want, N + Kw + nkp * nx, kappa)

