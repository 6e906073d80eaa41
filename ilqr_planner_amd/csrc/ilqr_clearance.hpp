// ilqr_clearance.hpp -- launchers of the clearance kernels (ilqr_problem_clearance, ilqr_clearance_trajectories; include/ilqr_hip.h "clearance");
// their definitions are ilqr_clearance_kernels.hpp, which ilqr_capi_kernels.cpp includes.
//
// Three launches per call: the per-state kernel writes one key (clearance, sphere, obstacle) per (trajectory, step) into a workspace, k_clr_fold
// folds the keys of a trajectory in ascending step order, k_clr_stats reduces clr_min per group.  Offsets are size_t (n T n_x may pass 2^31); a
// trajectory index is an int.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ilqr_hip.h"

namespace ilqr {

// The geometry of a call as the kernels read it: the descriptor's segments as they are (the kernel walks them; nothing is folded) and the robot's
// spheres and planes.  It lies in device memory -- with 32 spheres it is far beyond what kernel arguments hold -- and every lane reads it at
// wave-uniform addresses.
struct ClrGeom {
    int n_seg, n_walk;   // segments of the chain; segments the walk visits (up to the last sphere's link)
    int n_sph, n_planes;
    int seg_joint[ILQR_MAX_SEG];
    double seg_xyz[ILQR_MAX_SEG][3];
    double seg_R[ILQR_MAX_SEG][9];
    double seg_axis[ILQR_MAX_SEG][3];
    int sph_link[ILQR_CLR_MAX_SPH];
    double sph_c[ILQR_CLR_MAX_SPH][3];
    double sph_r[ILQR_CLR_MAX_SPH];
    double plane_n[ILQR_CLR_MAX_PLANES][3];
    double plane_d[ILQR_CLR_MAX_PLANES];
    // The self pairs as the walk uses them (clr_fill_geom).  The distinct first members are the anchors, slots 0 .. n_anchor-1 in ascending sphere
    // order; the walk keeps their world centres until it reaches the second members.
    int n_self, n_anchor;
    int self_slot[ILQR_CLR_MAX_SPH];    // the anchor slot of a sphere, or -1
    int self_mask[ILQR_CLR_MAX_SPH];    // bit t: the sphere is the second member of a pair with anchor slot t
    int anc_sph[ILQR_CLR_MAX_ANCHOR];   // the anchor's sphere index a
    int anc_first[ILQR_CLR_MAX_ANCHOR]; // the first joint behind the anchor's link: the joints m >= anc_first move b and not a
    double anc_r[ILQR_CLR_MAX_ANCHOR];  // r_a
};

// W[t] = w where t == slot; t[3] = W[slot]: an anchor's centre written and read by unrolled compares against the wave-uniform slot, so that W
// stays in registers (the idiom of obs_state's A[m] / O[m]).
__device__ __forceinline__ void clr_anchor_put(double (*W)[3], int slot, double wx, double wy, double wz) {
#pragma unroll
    for (int t = 0; t < ILQR_CLR_MAX_ANCHOR; t++)
        if (t == slot) { W[t][0] = wx; W[t][1] = wy; W[t][2] = wz; }
}
__device__ __forceinline__ void clr_anchor_get(const double (*W)[3], int slot, double* c) {
    c[0] = c[1] = c[2] = 0;
#pragma unroll
    for (int t = 0; t < ILQR_CLR_MAX_ANCHOR; t++)
        if (t == slot) { c[0] = W[t][0]; c[1] = W[t][1]; c[2] = W[t][2]; }
}

// Where the trajectories, the obstacles and the workspace of a call lie
struct ClrArgs {
    const ClrGeom* geom;
    const double* obs;    // [n_sets][n_obs][4]
    int n, T, n_obs, traj_per_set;
    double* ws_clr;       // [n T] the clearance of every (trajectory, step), NaN on a bad step
    int* ws_code;         // [n T] sphere | obstacle << 5 of the step's minimum, -1 without one
    int qrow[7];          // the row of joint j's position within a state (private layout: through the index map of a narrow chain)
    int n_anchor;         // host: the geometry's anchors; > 0 launches the self forms of the per-state kernels
};

// C = A B on row-major 3 x 3 matrices, one rounding per operation: the walks of clr_state and obs_state (ilqr_obstacle.hpp) share it
__device__ __forceinline__ void clr_mul(const double* A, const double* B, double* C) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

constexpr int CLR_MAX_OBS = (1 << 26) - ILQR_CLR_MAX_PLANES;   // the obstacle index shares an int with the sphere's

// k_clr_plan: the plan of a problem where it lies, X0 / X1 [T][NX][Bp] chosen per instance by cur; key of (b, k) at ws[k n + b]
void launch_clr_plan(const double* X0, const double* X1, const int* cur, int NX, int Bp, const ClrArgs& a, hipStream_t st);
// k_clr_traj: X[n][T][n_x] in the natural layout; key of (i, k) at ws[i T + k]
void launch_clr_traj(const double* X, int n_x, const ClrArgs& a, hipStream_t st);
// k_clr_fold: the keys of every trajectory in ascending step order -> clr_min, clr_at, n_below, eligible, clr (each may be null); the key of
// (i, k) lies at ws[i stride_i + k stride_k].  Afterwards ws_clr[i stride_i] holds clr_min of trajectory i (what k_clr_stats reads).
void launch_clr_fold(const ClrArgs& a, size_t stride_i, size_t stride_k, double margin, const ilqr_clr_out& out, hipStream_t st);
// k_clr_stats: stats[g] = { mean, min, n_hit, n_bad } over src[(g group + s) stride], s = 0 .. group-1
void launch_clr_stats(const double* src, size_t stride, int n_groups, int group, double margin, double* stats, hipStream_t st);

}  // namespace ilqr
