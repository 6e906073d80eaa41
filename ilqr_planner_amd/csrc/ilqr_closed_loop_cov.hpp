// ilqr_closed_loop_cov.hpp -- analytic propagation of the closed-loop state covariance (ilqr_problem_closed_loop_cov): the arguments and the
// step's Jacobian shared by the generic kernel (k_cl_cov, ilqr_kernels.hip) and the row kernel (k_cl_cov_rows, ilqr_closed_loop_cov.hip).
//
//   Sigma_0 = diag(sigma_x0^2),   Sigma_{k+1} = F_k Sigma_k F_k' + diag(sigma_w^2),   F_k = A_k + B_k K_k
// A_k, B_k are the Jacobian of dyn_step<S> at the plan (xbar_k, ubar_k); neither is formed.  With b_r the coefficient of row r's own control
// (dt on the joint rows of a 1st-order system; dt^2/2 on the position rows and dt on the velocity rows of a 2nd-order one; 0 on the time row),
// i(r) that control and c_r the row's entry in the time column of B (cov_time_col), both kernels evaluate
//   G = K Sigma                                                                       [n_u x n_x]   (u_var = the diagonal of G K')
//   M[r] = Sigma[r] (+ dt Sigma[7 + r] on the position rows, 2nd order) + b_r G[i(r)] + c_r G[last]                      = (F Sigma)[r]
//   H = M K'                                                                          [n_x x n_u]
//   Sigma'[r][c] = M[r][c] (+ dt M[r][7 + c] on the position columns) + b_c H[r][i(c)] + c_c H[r][last] (+ sigma_w[r]^2 on the diagonal)
// which is F Sigma F' with 2 n_u n_x^2 multiplications in place of 2 n_x^3.  The time column is NOT StepAB::bc (ilqr_batch_dev.hpp): that one
// reproduces the reference's B, which on PosOrnTime-2 uses the velocity after the step.
// The kernels sum in different orders (the generic one over the lower triangle, the row kernel over whole rows by lane): their results agree
// to rounding, not bit for bit.
#pragma once
#include "../../include/ilqr_hip.h"
#include "ilqr_closed_loop_plan.hpp"
#include "ilqr_kernels.hpp"

namespace ilqr {

struct ClCovArgs {
    double sw2[MAX_NX + 1] = {}, sx02[MAX_NX + 1] = {};   // sigma_w^2, sigma_x0^2 by DEVICE state entry (0 on the padding of a narrow chain)
    // natural layouts on the user's dimensions; each may be null
    double* Sigma = nullptr;     // [B][T][n_x][n_x]
    double* kp_Sigma = nullptr;  // [B][n_kp][n_x][n_x]
    double* u_var = nullptr;     // [B][T-1][n_u]
    double* lim_z = nullptr;     // [B]
    // ilqr_problem_closed_loop_cov_con: both null in every other call, and the kernels then do not look at the constraint rows (a.conA, a.conb)
    double* con_var = nullptr;   // [B][T-1][m]: c' Sigma_k c, c = A_k[r][0:n_x]' + K_k' A_k[r][n_x:]'
    double* con_z = nullptr;     // [B]
    double* ws = nullptr;        // generic kernel: [cl_cov_ws_entries][Bp] matrices of a step (entry e of instance b at ws[e Bp + b])
};

// entry of row `r` in the column of B for the time control s (dt = s^2): d dyn_step / d s at (x, u).  v: the velocity BEFORE the step.
template <int ND>
__host__ __device__ inline double cov_time_col(bool is_q, bool is_v, bool is_t, double dts, double u_i, double v_i) {
    if (is_t) return 2 * dts;
    if (ND == 1) return is_q ? 2 * dts * u_i : 0.0;
    if (is_q) return 2 * dts * v_i + 2 * dts * dts * dts * u_i;
    return is_v ? 2 * dts * u_i : 0.0;
}

int cl_cov_ws_entries(int kind, int nd);  // doubles per instance of k_cl_cov's workspace
// k_cl_cov (ilqr_kernels.hip); m: the maps of a chain of fewer than 7 joints, or null
void launch_closed_loop_cov(int kind, int nd, const Bufs& a, const ClCovArgs& c, int B, const DofMap* m, hipStream_t st);
// k_cl_cov_rows (ilqr_closed_loop_cov.hip), 7-joint layouts only.  A weak declaration, like launch_closed_loop_coop: the host builds of the
// generic kernel set link without that file.
__attribute__((weak)) void launch_closed_loop_cov_rows(int kind, int nd, const Bufs& a, const ClCovArgs& c, int B, hipStream_t st);
// k_cl_cov_kp (ilqr_kernels.hip), after either: kp_var[B][n_kp][ILQR_CL_COV_KP] of kp_Sigma; dof: the user's joints
void launch_closed_loop_cov_kp(int kind, int nd, const Bufs& a, int B, int n_kp, int dof, const double* kp_Sigma, double* kp_var, hipStream_t st);

}  // namespace ilqr
