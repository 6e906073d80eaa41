// ilqr_obstacle.hpp -- the sphere-obstacle terms of the stage cost (include/ilqr_hip.h "obstacle terms"): the per-state function, the argument
// block of the kernels that call it and their launchers.  The kernels themselves are in ilqr_kernels.hip (k_obs_derivs, k_obs_query, and the OBS
// forms of the generic k_init_rollout / k_backward / k_forward, and, compiled with ilqr_capi_kernels.cpp, k_stage_dense, k_obs_ls, k_obs_ls_sum of the
// cooperative path: ilqr_obstacle_coop_kernels.hpp); of the cooperative kernels only k_backward_si_dpp<.., SW_DENSE> takes them, as precomputed stage derivatives (ilqr_plan.hpp:
// PlanIn::obstacles_coop).
//
//   obs_state<WITH_DERIVS>   THE per-state function: clr_state's walk (ilqr_clearance_kernels.hpp: the segments as they are, the spheres by a
//                            cursor, a joint position loaded through a functor when the walk reaches its joint), with the hinge on every pair in
//                            place of the minimum.  Contraction is off and the cost's operations do not depend on WITH_DERIVS, so the derivative
//                            kernel, the rollouts and the query give the same cost bits for the same state.
// With derivatives it keeps the world axis and origin of the joints passed so far and accumulates sum h grad (7) and the upper triangle of
// sum grad grad' (28).  Every array is indexed by unrolled constants: joint m is stored by a compare against the (wave-uniform) joint index, and a
// joint the walk has not reached has a zero axis, so its gradient entry is 0 exactly -- nothing is indexed by a run-time value, nothing goes to
// scratch.  A self pair (a, b) is added at sphere b behind its planes: the anchors' centres wait in W[8][3] (clr_anchor_put / clr_anchor_get), and
// the gradient entries of the joints before the anchor's link are the literal 0 (ClrGeom::anc_first).  Moving joints are numbered 0 .. dof-1 in
// chain order (lower_chain refuses anything else) and joint j's position is row j of a device state for every chain (ilqr_dofmap.hpp), so entry m
// of the sums is device state entry m and a narrow chain's padded joints get nothing.
#pragma once
#include "ilqr_clearance.hpp"

namespace ilqr {

struct Bufs;      // ilqr_kernels.hpp
struct FwdArgs;   // ilqr_kernels.hpp

constexpr int OBS_LX = 1, OBS_LXX = 8, OBS_W = 36;   // a slot of obd: cost | sum over pairs of l_x (7) | upper triangle of l_xx by rows (28)
__host__ __device__ constexpr int obs_tri(int i, int j) { return i * 7 - i * (i - 1) / 2 + (j - i); }   // i <= j < 7

// What the kernels need of a problem's obstacle terms.  geom and obs are device memory the problem owns.
struct ObsArgs {
    const ClrGeom* geom;
    const double* obs;   // [n_sets][n_obs][4]; instance b reads set b / traj_per_set
    double* obd;         // [T][OBS_W][Bp]: the slot of step k of the current trajectory (k_obs_derivs)
    int n_obs, traj_per_set;
    double margin, weight;
};
struct ObsSelfArgs : ObsArgs {};   // the same block as the argument of the OBS forms of k_init_rollout / k_forward for a geometry with self pairs
// What a problem holds: the kernels' block and, for the host alone, the number of anchors of the geometry.  With n_anchor > 0 the problem is
// launched on the self forms (obs_state<.., true>) of the kernels that evaluate the terms; ObsArgs itself, a kernel argument, keeps its layout.
struct ObsProblem : ObsArgs { int n_anchor = 0; };

// q(j): the position of joint j of this lane's state.  obs: this instance's set.  Returns c_obs; with derivatives lx[7] = the term's l_x and
// lxx[28] = the upper triangle of its l_xx.
// SELF: the form with the self pairs; the launchers take it only for a geometry that has them (ObsProblem::n_anchor), so a geometry without
// runs the code it ran before there were any.
template <bool WITH_DERIVS, bool SELF = false, class Q>
__device__ __forceinline__ double obs_state(const ClrGeom& g, const double* __restrict__ obs, int n_obs, double margin, double weight, Q q, double* lx,
                                            double* lxx) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    double A[WITH_DERIVS ? 7 : 1][3], O[WITH_DERIVS ? 7 : 1][3];   // world axis and origin of joint m; zero until the walk reaches it
    if (WITH_DERIVS) {
#pragma unroll
        for (int m = 0; m < 7; m++) {
#pragma unroll
            for (int i = 0; i < 3; i++) A[m][i] = O[m][i] = 0;
            lx[m] = 0;
        }
#pragma unroll
        for (int e = 0; e < 28; e++) lxx[e] = 0;
    }
    double W[SELF ? ILQR_CLR_MAX_ANCHOR : 1][3];   // the anchors' centres (self pairs); a slot is written before any pair reads it
    if (SELF) {
#pragma unroll
        for (int t = 0; t < ILQR_CLR_MAX_ANCHOR; t++) W[t][0] = W[t][1] = W[t][2] = 0;
    }
    const int n_anchor = SELF ? g.n_anchor : 0;
    double sum = 0;
    bool bad = false;
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
                if (WITH_DERIVS) {
                    const double wa[3] = {(Rn[0] * ax + Rn[1] * ay) + Rn[2] * az, (Rn[3] * ax + Rn[4] * ay) + Rn[5] * az, (Rn[6] * ax + Rn[7] * ay) + Rn[8] * az};
#pragma unroll
                    for (int m = 0; m < 7; m++)
                        if (m == jn) {
#pragma unroll
                            for (int i = 0; i < 3; i++) { A[m][i] = wa[i]; O[m][i] = p[i]; }
                        }
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
                int first = 0;   // the first joint whose gradient entry is computed: the joints before it get a literal 0
                if (j < n_obs) {
                    const double oR = obs[4 * (size_t)j + 3];
                    if (oR < 0) continue;   // an unused slot
                    const double dx = w[0] - obs[4 * (size_t)j], dy = w[1] - obs[4 * (size_t)j + 1], dz = w[2] - obs[4 * (size_t)j + 2];
                    const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
                    d = (dist - r) - oR;
                    if (WITH_DERIVS) {   // a centre exactly on the obstacle's has no direction: its cost and a zero gradient
                        n[0] = dist > 0 ? dx / dist : 0.0;
                        n[1] = dist > 0 ? dy / dist : 0.0;
                        n[2] = dist > 0 ? dz / dist : 0.0;
                    }
                } else if (!SELF || j < n_pairs) {
                    const int l = j - n_obs;
                    d = ((((g.plane_n[l][0] * w[0] + g.plane_n[l][1] * w[1]) + g.plane_n[l][2] * w[2])) - g.plane_d[l]) - r;
                    if (WITH_DERIVS) { n[0] = g.plane_n[l][0]; n[1] = g.plane_n[l][1]; n[2] = g.plane_n[l][2]; }
                } else if constexpr (SELF) {
                    const int t = j - n_pairs;
                    if (!(mask >> t & 1)) continue;
                    double c[3];
                    clr_anchor_get(W, t, c);
                    const double dx = w[0] - c[0], dy = w[1] - c[1], dz = w[2] - c[2];
                    const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
                    d = (dist - r) - g.anc_r[t];
                    if (WITH_DERIVS) {   // coincident centres: the cost and a zero gradient; the joints before the anchor's link move both spheres rigidly
                        n[0] = dist > 0 ? dx / dist : 0.0;
                        n[1] = dist > 0 ? dy / dist : 0.0;
                        n[2] = dist > 0 ? dz / dist : 0.0;
                        first = g.anc_first[t];
                    }
                }
                const double h = margin - d;
                if (h > 0) {
                    sum = sum + h * h;
                    if (WITH_DERIVS) {
                        double gr[7];   // grad = n' Jp, column m of Jp = a_m x (p_i - r_m)
#pragma unroll
                        for (int m = 0; m < 7; m++) {
                            const double e0 = w[0] - O[m][0], e1 = w[1] - O[m][1], e2 = w[2] - O[m][2];
                            const double c0 = A[m][1] * e2 - A[m][2] * e1, c1 = A[m][2] * e0 - A[m][0] * e2, c2 = A[m][0] * e1 - A[m][1] * e0;
                            gr[m] = !SELF || m >= first ? (n[0] * c0 + n[1] * c1) + n[2] * c2 : 0.0;
                            lx[m] = lx[m] + h * gr[m];
                        }
#pragma unroll
                        for (int i = 0; i < 7; i++)
#pragma unroll
                            for (int jj = i; jj < 7; jj++) lxx[obs_tri(i, jj)] = lxx[obs_tri(i, jj)] + gr[i] * gr[jj];
                    }
                }
            }
            if constexpr (SELF) if (n_anchor) clr_anchor_put(W, g.self_slot[cur], w[0], w[1], w[2]);
        }
    }
    if (WITH_DERIVS) {
#pragma unroll
        for (int m = 0; m < 7; m++) lx[m] = -(weight * lx[m]);
#pragma unroll
        for (int e = 0; e < 28; e++) lxx[e] = weight * lxx[e];
    }
    return bad ? (double)NAN : weight * sum;
}

// k_obs_derivs: the slot obd[k] of every step of every instance's current trajectory (all = 0: of the active instances only, as k_kp_derivs),
// lanes along the batch, one grid row per step.  nx: rows of a device state.
void launch_obs_derivs(const Bufs& a, const ObsArgs& o, int B, int T, int nx, int all, hipStream_t st);
// The forms of a geometry with self pairs (ObsProblem::n_anchor > 0), which the caller picks; all of them are compiled with ilqr_capi_kernels.cpp, beside
// the cooperative obstacle kernels (ilqr_obstacle_coop_kernels.hpp), and none in ilqr_kernels.hip.
// k_obs_derivs_self: k_obs_derivs with obs_state<true, true>
void launch_obs_derivs_self(const Bufs& a, const ObsArgs& o, int B, int T, int nx, int all, hipStream_t st);
// k_init_rollout / k_forward<.., ObsSelfArgs> (ilqr_rollout_kernels.hpp): launch_init / launch_forward_generic with obs_state<false, true> inlined
void launch_init_self(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st, double penalty, const ObsArgs& o);
void launch_forward_generic_self(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st, const FwdArgs& f, const ObsArgs& o);
// k_obs_query: obd -> cost[B][T], lx[B][T][dof], lxx[B][T][dof][dof] (each may be null)
void launch_obs_query(const ObsArgs& o, int B, int Bp, int T, int dof, double* cost, double* lx, double* lxx, hipStream_t st);

// ---- the cooperative path of the single-integrator systems (RiccatiPlan::obs_dense; a device state is the 7 joint positions)
// Device memory the problem owns, allocated at the first solve on this path.
constexpr int OBS_LS_ROWS = 16;   // step sizes a line search of this path can hold (forward_wave_supported)
struct ObsDense {
    double* sd;     // [T][7 + 49][Bp]: l_x | l_xx (by rows) of every stage of the current trajectory, the element layout of one entry of Bufs::kpd
    double* part;   // [T][OBS_LS_ROWS][Bp]: c_obs of step k at step size index i of the line search in flight (k_obs_ls -> k_obs_ls_sum)
};
// k_stage_dense: sd[k] of every step of every instance the sweep visits (all = 0: the active ones), behind launch_kp_derivs and launch_obs_derivs.
// One fixed order per entry: base + obstacle term, where base is the entry of kpd at a keypoint step (limits already in it) and the limit terms
// (inspectJointLimit, the expressions of k_backward_si_dpp) at any other step, and the obstacle term is obd[k] with l_xx mirrored from its triangle.
void launch_stage_dense(const Bufs& a, const ObsArgs& o, double* sd, int B, int T, int all, hipStream_t st);
// k_obs_ls + k_obs_ls_sum.  init = 0, between the rollout of a line search and k_select: c_obs at x(alpha)_k for every step k and every step size
// index i < n_alpha of the active instances, x(alpha) = x(1) at i = 0 and fma(2^-i, x(1) - xbar, xbar) beyond (k_apply's expression; xbar = X[cur],
// x(1) = X[1 - cur]); then Bufs::lsc[i][b] += sum over k ascending, one lane per (instance, i): the order depends on T alone.
// init = 1, behind k_init_finish: one step size at xbar; cost[b] += that sum and status[b] is formed again from the cost.
void launch_obs_ls(const Bufs& a, const ObsProblem& o, double* part, int B, int T, int nx, int n_alpha, int init, hipStream_t st);

}  // namespace ilqr
