"""The device-pointer variants of a 6-joint problem on torch tensors (run by tests/test_gpu_narrow_chain.py in a process of its own, torch's
device initialised first): *_dev setters, getters and track_dev are bit-identical to the host-pointer calls; warm_start followed by track
matches the hand-padded 7-joint problem."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.init()

from ilqr_planner_amd import capi, workloads  # noqa: E402
from tests import narrow_chain as nc  # noqa: E402

DOF, B, NIT = 6, 96, 4


def main():
    ctx = capi.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    cfg, desc, inp, desc7, inp7 = nc.make_pair(ctx, "C2", DOF, B)
    cfg = dict(cfg)
    dev = torch.device("cuda")
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ph = workloads.load_batch(ctx, desc, inp, B)
    pd = capi.BatchProblem(ctx, desc, B)
    q0, dq0, U0 = tt(inp["q0"]), tt(inp["dq0"]), tt(inp["U0"])
    tg = [tt(t) for t in inp["targets"]]
    torch.cuda.synchronize()
    pd.set_init_state_dev(q0.data_ptr(), dq0.data_ptr())
    for k, t in enumerate(tg):
        pd.set_keypoint_targets_dev(k, t.data_ptr())
    pd.set_controls_dev(U0.data_ptr())
    for p in (ph, pd):
        workloads.run_solver(p, cfg, nb_iter=NIT, early_stop=False)
    T, nx, nu = cfg["T"], ph.dims.n_x, ph.dims.n_u
    assert (nx, nu) == (DOF, DOF)
    X, U = torch.empty((B, T, nx), dtype=torch.float64, device=dev), torch.empty((B, T - 1, nu), dtype=torch.float64, device=dev)
    pd.get_X_dev(X.data_ptr())
    pd.get_U_dev(U.data_ptr())
    ctx.synchronize()
    assert np.array_equal(X.cpu().numpy(), ph.X()) and np.array_equal(U.cpu().numpy(), ph.U())
    assert np.array_equal(pd.X(), ph.X()) and np.array_equal(pd.K(), ph.K()) and np.array_equal(pd.cost(), ph.cost())
    xm = np.random.default_rng(0).normal(0, 0.01, (B, nx)) + ph.X()[:, 3]
    u_h = ph.track(3, xm, True)
    xd, ud = tt(xm), torch.empty((B, nu), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.check(pd.L.ilqr_problem_track_dev(pd.h, 3, xd.data_ptr(), 1, ud.data_ptr()))
    ctx.synchronize()
    assert np.array_equal(ud.cpu().numpy(), u_h)
    print("dev variants: setters, getters and track_dev match the host-pointer calls", flush=True)
    # warm start + track against the hand-padded 7-joint problem
    p7 = workloads.load_batch(ctx, desc7, inp7, B)
    workloads.run_solver(p7, cfg, nb_iter=NIT, early_stop=False)
    xmap, umap, nx7, nu7 = nc.maps(cfg["kind"], cfg["nb_deriv"], DOF)
    for p in (ph, p7):
        p.warm_start(2)
        workloads.run_solver(p, cfg, nb_iter=2, early_stop=False)
    nc.assert_embedded(nc.results(ph, 2), nc.results(p7, 2), cfg["kind"], cfg["nb_deriv"], DOF)
    x7 = np.zeros((B, nx7))
    x7[:, xmap] = xm
    assert np.array_equal(ph.track(5, xm, True), p7.track(5, x7, True)[:, umap])
    for p in (ph, pd, p7):
        p.close()
    ctx.close()
    print("dev variants: ok")


if __name__ == "__main__":
    main()
