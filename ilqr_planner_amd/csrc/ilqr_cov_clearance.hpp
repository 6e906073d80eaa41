// ilqr_cov_clearance.hpp -- the clearance pairs under the closed-loop covariance (ilqr_problem_closed_loop_cov_clr; include/ilqr_hip.h "Analytic:
// ilqr_problem_closed_loop_cov_clr"): the per-state function, the argument block of its kernels and their launchers.  The kernels are
// ilqr_cov_clearance_kernels.hpp, compiled with ilqr_capi_kernels.cpp, so the host build of tests/tools/hostsim runs the same text.
//
//   cov_clr_state<SELF>   THE per-state function: the walk of obs_state<true, SELF> (ilqr_obstacle.hpp: the segments as they are, the spheres by a
//                         cursor, a joint position loaded through a functor when the walk reaches its joint, world axis and origin of the joints
//                         passed so far, the anchors' centres in registers) with, in place of the l_x / l_xx sums, the 28 entries of the upper
//                         triangle of Sigma_k[q,q].  Per pair it forms grad, var = grad' Sigma grad and z, and keeps the minimum in z.
// The walk is written here a third time (clr_state, obs_state, this): obs_state's template would have to grow a third mode, and every kernel that
// inlines it (k_obs_derivs, the OBS forms of the rollouts, k_obs_ls) would be compiled from changed text.  Their code objects stay what they were.
// Every array is indexed by unrolled constants, as in obs_state: nothing is indexed by a run-time value, nothing goes to scratch.
#pragma once
#include "ilqr_clearance.hpp"

namespace ilqr {

// the minimum of a step: a bad step (NaN, NaN, -1); a step without a pair, or whose pairs all have z = +inf: (+inf, 0, -1)
struct CovClrKey { double z, var; int code; };   // code: sphere | pair << 5

__host__ __device__ constexpr int cov_clr_tri(int i, int j) { return i * 7 - i * (i - 1) / 2 + (j - i); }   // i <= j < 7

// Where the plan's geometry, the covariance and the workspace of a call lie
struct CovClrArgs {
    const ClrGeom* geom;
    const double* obs;     // [n_sets][n_obs][4]
    const double* Sigma;   // [n][T][n_x][n_x], the natural layout on the user's dimensions
    int n, T, n_obs, traj_per_set, n_x, dof;   // n_x, dof: the user's
    double margin;
    double* ws_z;          // [T][n] z of the minimum of every (step, instance), NaN on a bad step
    double* ws_var;        // [T][n] its variance
    int* ws_code;          // [T][n] sphere | pair << 5, -1 without one
    int qrow[7];           // the row of joint j's position within a device state
    int n_anchor;          // host: the geometry's anchors; > 0 launches the self form
};

// q(j): the position of joint j of this lane's state.  obs: this instance's set.  S: the upper triangle of Sigma_k[q,q] by rows (cov_clr_tri),
// zero on the joints the chain does not have; sig_bad: an entry of it is not finite.
template <bool SELF, class Q>
__device__ __forceinline__ CovClrKey cov_clr_state(const ClrGeom& g, const double* __restrict__ obs, int n_obs, double margin, Q q, const double* S,
                                                   bool sig_bad) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    double A[7][3], O[7][3];   // world axis and origin of joint m; zero until the walk reaches it
#pragma unroll
    for (int m = 0; m < 7; m++) {
#pragma unroll
        for (int i = 0; i < 3; i++) A[m][i] = O[m][i] = 0;
    }
    double W[SELF ? ILQR_CLR_MAX_ANCHOR : 1][3];   // the anchors' centres (self pairs); a slot is written before any pair reads it
    if (SELF) {
#pragma unroll
        for (int t = 0; t < ILQR_CLR_MAX_ANCHOR; t++) W[t][0] = W[t][1] = W[t][2] = 0;
    }
    const int n_anchor = SELF ? g.n_anchor : 0;
    CovClrKey key{INFINITY, 0.0, -1};
    bool bad = sig_bad;
    int cur = 0;
    const int n_sph = g.n_sph, n_pairs = n_obs + g.n_planes;
#pragma unroll 1
    for (int s = -1; s < g.n_walk; s++) {   // link -1 is the base: its spheres come before the first segment
        if (s >= 0) {
            const double x = g.seg_xyz[s][0], y = g.seg_xyz[s][1], z = g.seg_xyz[s][2];
#pragma unroll
            for (int i = 0; i < 3; i++) p[i] = p[i] + ((R[3 * i] * x + R[3 * i + 1] * y) + R[3 * i + 2] * z);
            double Rn[9];
            clr_mul(R, g.seg_R[s], Rn);
            const int jn = g.seg_joint[s];   // wave-uniform
            if (jn >= 0) {
                const double qj = q(jn);
                bad = bad || !isfinite(qj);
                const double ax = g.seg_axis[s][0], ay = g.seg_axis[s][1], az = g.seg_axis[s][2];
                const double wa[3] = {(Rn[0] * ax + Rn[1] * ay) + Rn[2] * az, (Rn[3] * ax + Rn[4] * ay) + Rn[5] * az, (Rn[6] * ax + Rn[7] * ay) + Rn[8] * az};
#pragma unroll
                for (int m = 0; m < 7; m++)
                    if (m == jn) {
#pragma unroll
                        for (int i = 0; i < 3; i++) { A[m][i] = wa[i]; O[m][i] = p[i]; }
                    }
                double st, ct;
                sincos(qj, &st, &ct);
                const double vt = 1 - ct;
                const double Rq[9] = {ct + vt * ax * ax,      -az * st + vt * ax * ay, ay * st + vt * ax * az,
                                      az * st + vt * ax * ay, ct + vt * ay * ay,       -ax * st + vt * ay * az,
                                      -ay * st + vt * ax * az, ax * st + vt * ay * az, ct + vt * az * az};
                clr_mul(Rn, Rq, R);
            } else {
#pragma unroll
                for (int i = 0; i < 9; i++) R[i] = Rn[i];
            }
        }
#pragma unroll 1
        for (; cur < n_sph && g.sph_link[cur] == s; cur++) {
            const double cx = g.sph_c[cur][0], cy = g.sph_c[cur][1], cz = g.sph_c[cur][2], r = g.sph_r[cur];
            const double w[3] = {p[0] + ((R[0] * cx + R[1] * cy) + R[2] * cz), p[1] + ((R[3] * cx + R[4] * cy) + R[5] * cz),
                                 p[2] + ((R[6] * cx + R[7] * cy) + R[8] * cz)};
            const int mask = SELF && n_anchor ? g.self_mask[cur] : 0;   // wave-uniform: the anchors this sphere is paired with
#pragma unroll 1
            for (int j = 0; j < (SELF ? n_pairs + n_anchor : n_pairs); j++) {   // the obstacles of the set, then the planes, then the self pairs (anchors ascending)
                double d, n[3];
                int first = 0, pair = j;   // the first joint whose gradient entry is computed; the pair's number in the call's numbering
                if (j < n_obs) {
                    const double oR = obs[4 * (size_t)j + 3];
                    if (oR < 0) continue;   // an unused slot
                    const double dx = w[0] - obs[4 * (size_t)j], dy = w[1] - obs[4 * (size_t)j + 1], dz = w[2] - obs[4 * (size_t)j + 2];
                    const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
                    d = (dist - r) - oR;
                    n[0] = dist > 0 ? dx / dist : 0.0;   // a centre exactly on the obstacle's has no direction: a zero gradient
                    n[1] = dist > 0 ? dy / dist : 0.0;
                    n[2] = dist > 0 ? dz / dist : 0.0;
                } else if (!SELF || j < n_pairs) {
                    const int l = j - n_obs;
                    d = ((((g.plane_n[l][0] * w[0] + g.plane_n[l][1] * w[1]) + g.plane_n[l][2] * w[2])) - g.plane_d[l]) - r;
                    n[0] = g.plane_n[l][0]; n[1] = g.plane_n[l][1]; n[2] = g.plane_n[l][2];
                } else if constexpr (SELF) {
                    const int t = j - n_pairs;
                    if (!(mask >> t & 1)) continue;
                    double c[3];
                    clr_anchor_get(W, t, c);
                    const double dx = w[0] - c[0], dy = w[1] - c[1], dz = w[2] - c[2];
                    const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
                    d = (dist - r) - g.anc_r[t];
                    n[0] = dist > 0 ? dx / dist : 0.0;   // coincident centres: a zero gradient
                    n[1] = dist > 0 ? dy / dist : 0.0;
                    n[2] = dist > 0 ? dz / dist : 0.0;
                    first = g.anc_first[t];   // the joints before the anchor's link move both spheres rigidly: a literal 0
                    pair = n_pairs + g.anc_sph[t];
                }
                double gr[7];   // grad = n' Jp, column m of Jp = a_m x (p_i - r_m)
#pragma unroll
                for (int m = 0; m < 7; m++) {
                    const double e0 = w[0] - O[m][0], e1 = w[1] - O[m][1], e2 = w[2] - O[m][2];
                    const double c0 = A[m][1] * e2 - A[m][2] * e1, c1 = A[m][2] * e0 - A[m][0] * e2, c2 = A[m][0] * e1 - A[m][1] * e0;
                    gr[m] = !SELF || m >= first ? (n[0] * c0 + n[1] * c1) + n[2] * c2 : 0.0;
                }
                double form = 0;   // rows ascending, columns ascending within a row: (grad_i Sigma_ij) grad_j, one rounding per operation
#pragma unroll
                for (int i = 0; i < 7; i++)
#pragma unroll
                    for (int jj = 0; jj < 7; jj++) form = form + (gr[i] * S[i <= jj ? cov_clr_tri(i, jj) : cov_clr_tri(jj, i)]) * gr[jj];
                const double var = form > 0 ? form : 0.0;   // a form that rounding leaves below 0 counts as 0
                const double num = d - margin;
                const double z = var > 0 ? num / sqrt(var) : (d >= margin ? (double)INFINITY : -(double)INFINITY);
                if (z < key.z) { key.z = z; key.var = var; key.code = cur | (pair << 5); }
            }
            if constexpr (SELF) if (n_anchor) clr_anchor_put(W, g.self_slot[cur], w[0], w[1], w[2]);
        }
    }
    if (bad) { key.z = (double)NAN; key.var = (double)NAN; key.code = -1; }
    return key;
}

// k_cov_clr: the plan of a problem where it lies, X0 / X1 [T][NX][Bp] chosen per instance by cur, and Sigma_k of the covariance the call has just
// produced; the key of (b, k) at ws[k n + b]
void launch_cov_clr(const double* X0, const double* X1, const int* cur, int NX, int Bp, const CovClrArgs& a, hipStream_t st);
// k_cov_clr_fold: the keys of every plan in ascending step order -> clr_var, clr_z, clr_z_min, clr_z_at, eligible (each may be null)
void launch_cov_clr_fold(const CovClrArgs& a, double z_tol, const ilqr_cl_cov_clr& out, hipStream_t st);

}  // namespace ilqr
