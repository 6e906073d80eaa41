"""bench.py --dump-outputs on CPU: a stand-in for the solved problem (the getters of capi.BatchProblem) checks which arrays are written,
that they are float64 and indexed by instance, that a batch too large for the budget is cut to the same seeded sample in every array and
every run, and that the files stay within the budget."""
import os

import numpy as np

import bench


class _Dims:
    n_x, n_u, n_f = 7, 7, 7


class _Problem:
    """The getters bench.dump_outputs reads, filled with values that name their instance (entry [b, ...] = b + position / 1e6)."""

    def __init__(self, B, T):
        self.B, self.T, self.dims = B, T, _Dims()

    def _arr(self, *shape):
        a = np.arange(int(np.prod(shape[1:])), dtype=np.float64).reshape(shape[1:]) * 1e-6
        return np.arange(shape[0], dtype=np.float64).reshape((-1,) + (1,) * (len(shape) - 1)) + a[None]

    def X(self):
        return self._arr(self.B, self.T, self.dims.n_x)

    def fX(self):
        return self._arr(self.B, self.T, self.dims.n_f)

    def U(self):
        return self._arr(self.B, self.T - 1, self.dims.n_u)

    def K(self):
        return self._arr(self.B, self.T - 1, self.dims.n_u, self.dims.n_x)

    def d(self):
        return self._arr(self.B, self.T - 1, self.dims.n_u)

    def trace(self, nb_iter):
        return self._arr(self.B, nb_iter), self._arr(self.B, nb_iter)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


def test_whole_batch_when_it_fits(tmp_path):
    B, T, nb = 16, 20, 5
    p = _Problem(B, T)
    out = bench.dump_outputs(p, {"solver": "recursive"}, nb, np.arange(B, dtype=np.float64), str(tmp_path))
    got = _load(tmp_path)
    assert set(got) == {"instance_index", "cost", "X", "fX", "U", "K", "d", "cost_trace", "alpha_trace"} == set(out["arrays"])
    assert out["instances"] == B and all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["instance_index"], np.arange(B))
    np.testing.assert_array_equal(got["X"], p.X())
    np.testing.assert_array_equal(got["K"], p.K())
    np.testing.assert_array_equal(got["cost_trace"], p.trace(nb)[0])


def test_seeded_sample_within_budget(tmp_path):
    B, T, nb, budget = 512, 200, 20, 2 * 10**6
    p = _Problem(B, T)
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        out = bench.dump_outputs(p, {"solver": "al"}, nb, np.arange(B, dtype=np.float64), str(d), budget=budget)
        assert 0 < out["instances"] < B and out["bytes"] <= budget
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= budget
        runs.append(_load(d))
    a, b = runs
    assert set(a) == {"instance_index", "cost", "X", "fX", "U", "cost_trace", "alpha_trace"}  # AL-ILQR returns no gains
    for name in a:
        np.testing.assert_array_equal(a[name], b[name])  # the same sample in every run
    idx = a["instance_index"]
    assert len(np.unique(idx)) == len(idx) == len(a["cost"])
    for name in ("cost", "X", "fX", "U", "cost_trace"):
        np.testing.assert_array_equal(np.floor(a[name].reshape(len(idx), -1)[:, 0]), idx)  # every array holds the same instances
