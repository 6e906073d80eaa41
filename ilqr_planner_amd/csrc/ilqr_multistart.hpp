// ilqr_multistart.hpp -- launchers of the kernels that join instances (ilqr_problem_adopt, ilqr_problem_spread_controls, ilqr_problem_select,
// ilqr_problem_get_at); their definitions are ilqr_multistart_kernels.hpp, which ilqr_capi_kernels.cpp includes.
//
// Every other kernel of the library stays inside one instance; these four read or write across the batch.  Offsets: an instance index is an int
// (B < 2^31), every offset into a [row][Bp] buffer or a natural-layout array is formed as size_t (B T n may pass 2^31).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ilqr_hip.h"
#include "ilqr_dofmap.hpp"

namespace ilqr {

// k_adopt_rows: dst[r][b] = (cur && cur[i] ? s1 : s0)[r][i], i = index[b] clamped into 0 .. B_src-1, for b < B_dst and every row r < rows.
void launch_adopt_rows(const double* s0, const double* s1, const int* cur, const int* index, double* dst, int rows, int B_dst, int Bp_dst, int B_src,
                       int Bp_src, hipStream_t st);
// k_spread_controls: U0[k][dev(i)][b] += sigma_u[i] z for every member but the global member 0 of its group; u maps the user's control entries
// to device rows (the identity for 7 joints).
void launch_spread_controls(double* U0, int B, int Bp, int T1, int group_size, const ilqr_seeds& seeds, const IndexMap& u, hipStream_t st);
// k_select_group: winner / best / n_candidates of every group (each may be null); score is indexed by the instance (a natural [B] array and the
// problem's own cost buffer alike), eligible may be null.
void launch_select_group(const double* score, const int* eligible, const int* status, int G, int group_size, int* winner, double* best,
                         int* n_candidates, hipStream_t st);
// k_get_at: out[j][r] = (cur && cur[i] ? s1 : s0)[device row of r][i], i = index[j] clamped; m (null: the identity) narrows every per-step vector
// of `outer` vectors to the user's layout, rows = outer * (m ? m->n_user : width).
void launch_get_at(const double* s0, const double* s1, const int* cur, const int* index, double* out, int n, int B_src, int Bp_src, int rows,
                   const IndexMap* m, hipStream_t st);
// k_get_at<int, false>: out[j] = src[index[j] clamped]
void launch_get_at_int(const int* src, const int* index, int* out, int n, int B_src, hipStream_t st);

}  // namespace ilqr
