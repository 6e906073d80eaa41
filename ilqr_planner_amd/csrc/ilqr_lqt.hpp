// ilqr_lqt.hpp -- launchers of the batched linear-quadratic tracking kernels (ilqr_lqt.hip), used by the C ABI in ilqr_lqt.cpp.
// The math and the data layout are in ilqr_lqt.hip and DESIGN.md section 9.
#pragma once
#include <hip/hip_runtime.h>

namespace ilqr {

// Device buffers of one LQT handle.  `chains` is 1 when the precisions are shared by the batch, B when they are per instance.
struct LqtDev {
    int n = 0, m = 0, N = 0, B = 0, chains = 1;
    double r = 0;              // R = r I_m
    const double* A = nullptr;   // [n][n]
    const double* Bm = nullptr;  // [n][m]
    const double* Q = nullptr;   // [chains][N][n][n]; Q[N-1] is the terminal weight P_{N-1}
    const double* mu = nullptr;  // [B][N][n]
    double* P = nullptr;         // [chains][N][n][n]
    double* L = nullptr;         // [chains][N][m][n]   L_t = S_t^-1 B' P_t,  S_t = B' P_t B + R
    double* H = nullptr;         // [chains][N][m][n]   H_t = S_t^-1 B'
    double* W = nullptr;         // [N][n][n] (shared chain only): W_t = (A - B L_t A)', t >= 1
    double* d = nullptr;         // [B][N][n]
    double* U = nullptr;         // [B][N-1][m]
    double* X = nullptr;         // [B][N][n]
    double* dump = nullptr;      // [64]: target of the stores of lanes that own no entry (their values are never read)
};

// lanes per instance of the lane-group kernels: the smallest of 4, 8, 16 that holds max(n, m)
inline int lqt_group(int n, int m) {
    const int w = n > m ? n : m;
    return w <= 4 ? 4 : (w <= 8 ? 8 : 16);
}

void launch_lqt_chain(const LqtDev& a, hipStream_t s);        // k_lqt_chain: P, L, H (+ W shared, + d per instance)
void launch_lqt_affine(const LqtDev& a, hipStream_t s);       // k_lqt_affine: d of every instance from the shared chain
void launch_lqt_rollout(const LqtDev& a, hipStream_t s);      // k_lqt_rollout: U, X from x_0 = mu_0
void launch_lqt_command(const LqtDev& a, int tau, const double* x, double* u, hipStream_t s);  // k_lqt_command

}  // namespace ilqr
