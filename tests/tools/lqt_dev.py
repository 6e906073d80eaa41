"""The device-pointer variants of capi.LQTBatch on torch tensors (run by tests/test_gpu_lqt.py in a process of its own, torch's device
initialised first): set_targets_dev, command_dev, U_dev and X_dev are bit-identical to the host-pointer calls."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.cuda.init()

from ilqr_planner_amd import capi  # noqa: E402
from tests import lqt_reference as ref  # noqa: E402


def main():
    n, m, N, B = 6, 3, 25, 500
    rng = np.random.default_rng(3)
    A, Bm, Qs, _, r = ref.random_problem(rng, n, m, N)
    mu = rng.standard_normal((B, N, n))
    x = rng.standard_normal((B, n))
    ctx = capi.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lq = capi.LQTBatch(ctx, A, Bm, Qs, mu, r)
    lq.solve_lin_al()
    U, X, u = lq.U(), lq.X(), lq.command(2, x)
    lq.close()
    dev = torch.device("cuda")
    lq = capi.LQTBatch(ctx, A, Bm, Qs, np.zeros_like(mu), r)
    mu_t, xd = torch.from_numpy(mu).to(dev), torch.from_numpy(x).to(dev)
    Ud = torch.empty((B, N - 1, m), dtype=torch.float64, device=dev)
    Xd = torch.empty((B, N, n), dtype=torch.float64, device=dev)
    ud = torch.empty((B, m), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    lq.set_targets_dev(mu_t.data_ptr())
    lq.solve_lin_al()
    lq.U_dev(Ud.data_ptr())
    lq.X_dev(Xd.data_ptr())
    lq.command_dev(2, xd.data_ptr(), ud.data_ptr())
    ctx.synchronize()
    assert np.array_equal(Ud.cpu().numpy(), U)
    assert np.array_equal(Xd.cpu().numpy(), X)
    assert np.array_equal(ud.cpu().numpy(), u)
    lq.close()
    ctx.close()
    print("lqt dev variants: ok")


if __name__ == "__main__":
    main()
