// ilqr_cov_clearance_kernels.hpp -- the kernels of ilqr_problem_closed_loop_cov_clr: definitions and launchers, included by ilqr_capi_kernels.cpp
// alone (inside no namespace), for the reasons at the top of ilqr_clearance_kernels.hpp.  Plain C++ without lane communication: the host build
// runs the very same code.
//
//   k_cov_clr        lanes along the batch, steps on blockIdx.y, as k_clr_plan: the plan where it lies (every load of a wave is one whole
//                    512-byte run of a [row][Bp] row) and the upper triangle of Sigma_k[q,q] from the covariance in its natural layout
//                    (28 loads per lane, strided by n_x^2 doubles between lanes)
//   k_cov_clr_self   the same with cov_clr_state<true>, launched for a geometry with self pairs
//   k_cov_clr_fold   one lane per plan: its keys in ascending step order under the total order of include/ilqr_hip.h
// The workspace holds 20 bytes per (instance, step): z, the variance and sphere | pair << 5.
#pragma once
#ifndef ILQR_COV_CLEARANCE_KERNELS_TU
#error "ilqr_cov_clearance_kernels.hpp holds definitions with external linkage: one translation unit (ilqr_capi_kernels.cpp) defines ILQR_COV_CLEARANCE_KERNELS_TU and includes it; every other one includes ilqr_cov_clearance.hpp"
#endif
#include "ilqr_cov_clearance.hpp"

namespace ilqr {

template <bool SELF>
__device__ __forceinline__ void cov_clr_body(const double* __restrict__ X0, const double* __restrict__ X1, const int* __restrict__ cur, int NX, int Bp,
                                             int k0, const CovClrArgs& a) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int k = k0 + (int)blockIdx.y;
    if (b >= a.n) return;
    const double* x = (cur[b] ? X1 : X0) + (size_t)k * (size_t)NX * (size_t)Bp + (size_t)b;
    const size_t Bps = (size_t)Bp;
    const double* sg = a.Sigma + ((size_t)b * (size_t)a.T + (size_t)k) * (size_t)a.n_x * (size_t)a.n_x;
    double S[28];
    bool sig_bad = false;
#pragma unroll
    for (int i = 0; i < 7; i++)
#pragma unroll
        for (int j = i; j < 7; j++) {
            const double v = j < a.dof ? sg[(size_t)i * (size_t)a.n_x + (size_t)j] : 0.0;   // wave-uniform: the joints the chain has
            sig_bad = sig_bad || !isfinite(v);
            S[cov_clr_tri(i, j)] = v;
        }
    const CovClrKey key = cov_clr_state<SELF>(*a.geom, a.obs + (size_t)(b / a.traj_per_set) * (size_t)a.n_obs * 4, a.n_obs, a.margin,
                                              [&](int j) { return x[(size_t)a.qrow[j] * Bps]; }, S, sig_bad);
    const size_t w = (size_t)k * (size_t)a.n + (size_t)b;
    a.ws_z[w] = key.z;
    a.ws_var[w] = key.var;
    a.ws_code[w] = key.code;
}
__global__ __launch_bounds__(256) void k_cov_clr(const double* __restrict__ X0, const double* __restrict__ X1, const int* __restrict__ cur, int NX, int Bp,
                                                 int k0, CovClrArgs a) {
    cov_clr_body<false>(X0, X1, cur, NX, Bp, k0, a);
}
__global__ __launch_bounds__(256) void k_cov_clr_self(const double* __restrict__ X0, const double* __restrict__ X1, const int* __restrict__ cur, int NX,
                                                      int Bp, int k0, CovClrArgs a) {
    cov_clr_body<true>(X0, X1, cur, NX, Bp, k0, a);
}

// Steps ascend, so a strict `<` keeps the lowest step of equal z; sphere and pair were settled within the step.
__global__ __launch_bounds__(256) void k_cov_clr_fold(const double* __restrict__ ws_z, const double* __restrict__ ws_var, const int* __restrict__ ws_code,
                                                      int n, int T, double z_tol, ilqr_cl_cov_clr out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double best = INFINITY;
    int bk = 0, bcode = -1, badk = -1;
    for (int k = 0; k < T; k++) {
        const size_t w = (size_t)k * (size_t)n + (size_t)i;
        const double z = ws_z[w];
        if (out.clr_z) out.clr_z[(size_t)i * (size_t)T + (size_t)k] = z;
        if (out.clr_var) out.clr_var[(size_t)i * (size_t)T + (size_t)k] = ws_var[w];
        if (z != z) {
            if (badk < 0) badk = k;
        } else if (z < best) { best = z; bk = k; bcode = ws_code[w]; }
    }
    const bool bad = badk >= 0;
    if (out.clr_z_min) out.clr_z_min[i] = bad ? (double)NAN : best;
    if (out.clr_z_at) {
        int* at = out.clr_z_at + (size_t)i * 3;
        at[0] = bad ? badk : bk;
        at[1] = (bad || bcode < 0) ? -1 : (bcode & 31);
        at[2] = (bad || bcode < 0) ? -1 : (bcode >> 5);
    }
    if (out.eligible) out.eligible[i] = (!bad && best >= z_tol) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ launchers

void launch_cov_clr(const double* X0, const double* X1, const int* cur, int NX, int Bp, const CovClrArgs& a, hipStream_t st) {
    for (int k0 = 0; k0 < a.T; k0 += 65535) {   // the y extent of a grid
        const int rows = a.T - k0 < 65535 ? a.T - k0 : 65535;
        if (a.n_anchor) hipLaunchKernelGGL(k_cov_clr_self, dim3((a.n + 255) / 256, rows), dim3(256), 0, st, X0, X1, cur, NX, Bp, k0, a);
        else hipLaunchKernelGGL(k_cov_clr, dim3((a.n + 255) / 256, rows), dim3(256), 0, st, X0, X1, cur, NX, Bp, k0, a);
    }
}

void launch_cov_clr_fold(const CovClrArgs& a, double z_tol, const ilqr_cl_cov_clr& out, hipStream_t st) {
    hipLaunchKernelGGL(k_cov_clr_fold, dim3((a.n + 255) / 256), dim3(256), 0, st, (const double*)a.ws_z, (const double*)a.ws_var, (const int*)a.ws_code, a.n,
                       a.T, z_tol, out);
}

}  // namespace ilqr
