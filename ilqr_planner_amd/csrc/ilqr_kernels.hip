// ilqr_kernels.hip -- batched iLQR kernels for gfx950 (MI355X), fp64.
//
// v1 mapping: ONE LANE PER PROBLEM INSTANCE.  Trajectory/gain buffers are structure-of-arrays with the batch
// innermost ([t][component][Bp]) so every load/store of a wave is one contiguous 512-byte segment; all the small
// dense algebra of a timestep lives in that lane's registers.  The time recursion (rollout, Riccati sweep) is
// sequential inside the lane; parallelism is across instances only.
//
// Reference behaviour restated (paths relative to ilqr_planner/ilqr_planner in the reference tree):
//   initial rollout            src/solver/ILQRRecursive.cpp:27-56   (AL: src/solver/AL-ILQR.cpp:53-85)
//   backward Riccati sweep     src/solver/ILQRRecursive.cpp:68-97   (AL terms: src/solver/AL-ILQR.cpp:110-134)
//   forward pass + line search src/solver/ILQRRecursive.cpp:101-176 (AL: src/solver/AL-ILQR.cpp:149-227)
// A_k, B_k are never stored: they are rebuilt from (x_k, u_k) exactly as forwardPass builds them.
#include "ilqr_closed_loop.hpp"
#include "ilqr_closed_loop_cov.hpp"
#include "ilqr_kernels.hpp"
#include "ilqr_obstacle.hpp"
#include "ilqr_step.hpp"

namespace ilqr {

// ------------------------------------------------------------------------------------------------ kernels

#define NOUNR _Pragma("unroll 1")

// The obstacle term of a state inside the sequential kernels (the OBS forms of k_init_rollout / k_forward): obs_state<false> out of line, as
// kp_cost_call keeps the keypoint code out of their loops.  The joint positions travel by value and are picked by a compare chain on the
// (uniform) joint index: no private array is indexed.
__device__ __noinline__ double obs_cost_call(const ClrGeom* g, const double* obs, int n_obs, double margin, double weight, double q0, double q1, double q2,
                                             double q3, double q4, double q5, double q6) {
    return obs_state<false>(*g, obs, n_obs, margin, weight,
                            [&](int j) { return j == 0 ? q0 : j == 1 ? q1 : j == 2 ? q2 : j == 3 ? q3 : j == 4 ? q4 : j == 5 ? q5 : q6; }, nullptr, nullptr);
}
ILQR_DEV double obs_stage_cost(ObsArgs o, int b, const double* x) {
    return obs_cost_call(o.geom, o.obs + (size_t)(b / o.traj_per_set) * (size_t)o.n_obs * 4, o.n_obs, o.margin, o.weight, x[0], x[1], x[2], x[3], x[4], x[5], x[6]);
}

ILQR_DEV const double* obs_slot(ObsArgs o, int k, int Bp) { return o.obd + (size_t)k * OBS_W * (size_t)Bp; }

#include "ilqr_rollout_kernels.hpp"   // k_init_rollout, k_forward

// ilqr_problem_gains: what a sweep about the held plan needs that a solve's rollout would have set up.  Every instance is swept (the sweeps skip
// the instances an early stop made inactive; the next solve's rollout resets `active`), and the feed-forward it writes is unscaled: alpha = 1
// (the getters' and the tracking law's rule is iters > 0 ? alpha : 1).  Nothing else of the plan is touched.
__global__ __launch_bounds__(64) void k_gains_prepare(Bufs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.desc->B) return;
    a.active[b] = 1;
    a.alpha[b] = 1.0;
}

// ilqr_problem_gains_al: the active-set weights penalty * I_k of the held plan for the sweeps that read Is (AL-ILQR.cpp:21-44,190), one lane per
// (instance, step): g by con_g on X[cur], U[cur] -- the expression k_init_rollout and k_al_post evaluate on the same bytes, so the weights are the
// ones a fresh solve about this plan would form -- with the multipliers as they are.  Unlike k_al_post it looks at no iteration count and updates
// no multiplier: every instance gets its weights, and only Is is written.
template <class S>
__global__ __launch_bounds__(256) void k_gains_al_weights(Bufs a, double penalty) {
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (b >= d.B) return;
    const int Bp = d.Bp;
    const int cur = a.cur[b];
    double x[S::NX], u[S::NU];
    UNR for (int i = 0; i < S::NX; i++) x[i] = AT(a.X[cur], k * S::NX + i, b);
    UNR for (int i = 0; i < S::NU; i++) u[i] = AT(a.U[cur], k * S::NU + i, b);
    for (int r = 0; r < a.m; r++) {
        const double g = con_g<S>(a, k, r, x, u);
        const double lam = AT(a.lambda, k * a.m + r, b);
        AT(a.Is, k * a.m + r, b) = penalty * ((g < 0 && lam == 0) ? 0.0 : 1.0);
    }
}

// l_x, l_xx of the keypoint steps (System::cost_x / cost_xx incl. the limit terms) for the current trajectory, one lane per
// (instance, keypoint).  Keeps FK, the quaternion log map and J'QJ out of the sequential sweep: the sweep only loads
// NX + NX*NX doubles at the (two) keypoint steps.
template <class S, bool EXT>
__global__ __launch_bounds__(64) void k_kp_derivs(Bufs a, int fused) {
    constexpr int NX = S::NX;
    // origins and axes of the joints and the joint angles (7 x DOF per lane) for the rolled FK loop: a short launch between the streaming kernels is bound by
    // fetching its code, and the unrolled joints were most of it (ilqr_device.hpp: fk)
    constexpr int ROLLN = (!S::JOINT && S::ND == 1) ? 64 : 0;  // (2nd order: the rolled form spills more)
    __shared__ double sj[ROLLN ? 7 * DOF : 1][64];  // (nothing reserved where the loop is not rolled)
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x;
    const int kpi = blockIdx.y;
    if (b >= d.B) return;
    if (!a.active[b]) return;
    const int Bp = d.Bp;
    const int k = d.kp_t[kpi];
    const int cur = a.cur[b];
    const double* X = a.X[cur];
    double x[NX];
    UNR for (int i = 0; i < NX; i++) x[i] = AT(X, k * NX + i, b);
    const int w = fused ? a.pend[b] - 1 : -1;
    if (w >= 0) {  // fused acceptance (FwdArgs::fused): the accepted state is still spread over the two buffers -- k_apply's expression
        const double aa = ldexp(1.0, -w);
        const double* X1 = a.X[1 - cur];
        UNR for (int i = 0; i < NX; i++) {
            const double x1 = AT(X1, k * NX + i, b);
            x[i] = (w == 0) ? x1 : fma(aa, x1 - x[i], x[i]);
        }
    }
    // row by row straight to memory: the lane never holds the n_x x n_x matrix (it spilled for n_x = 14, 15)
    double* out = a.kpd + (size_t)kpi * (NX + NX * NX) * Bp;
    stage_derivs_rows<S, EXT, ROLLN>(d, a, b, x, kpi, &sj[0][threadIdx.x], [&](int i, const double* row, double lxi) {
        AT(out, i, b) = lxi;
        UNR for (int j = 0; j < NX; j++) AT(out, NX + i * NX + j, b) = row[j];
    });
}

// k_kp_derivs for problems whose keypoints share a timestep (ilqr_steps.hpp), in two launches.  k_kp_terms: one block column per KEYPOINT
// (as k_kp_derivs: the keypoint index is the uniform blockIdx.y), its l_x | l_xx without the limit terms into its own slot behind the steps'
// slots (kpd slot n_steps + keypoint).  k_kp_sum: one block column per distinct step, whose kpd slot receives the sum of its keypoints' slots in
// keypoint order (by sub-system index within a step: SequentialSystem.cpp:144-165 sums cost_x / cost_xx over the sub-systems), then the limit
// terms once.  (One kernel looping over a step's keypoints kept the FK and Jacobian code live across the loop: 2 KB of scratch on the
// 2nd-order systems.)  Only the generic kernels read these slots (plan_riccati routes shared steps there), so there is no fused acceptance.
template <class S>
__global__ __launch_bounds__(64) void k_kp_terms(Bufs a) {
    constexpr int NX = S::NX;
    constexpr int ROLLN = (!S::JOINT && S::ND == 1) ? 64 : 0;
    __shared__ double sj[ROLLN ? 7 * DOF : 1][64];
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x;
    const int kpi = blockIdx.y;
    if (b >= d.B) return;
    if (!a.active[b]) return;
    const int Bp = d.Bp;
    const int k = d.kp_t[kpi];
    const double* X = a.X[a.cur[b]];
    double x[NX];
    UNR for (int i = 0; i < NX; i++) x[i] = AT(X, k * NX + i, b);
    double* out = a.kpd + (size_t)(d.steps.n + kpi) * (NX + NX * NX) * Bp;
    stage_derivs_rows<S, true, ROLLN, false>(d, a, b, x, kpi, &sj[0][threadIdx.x], [&](int i, const double* row, double lxi) {
        AT(out, i, b) = lxi;
        UNR for (int j = 0; j < NX; j++) AT(out, NX + i * NX + j, b) = row[j];
    });
}

template <class S>
__global__ __launch_bounds__(64) void k_kp_sum(Bufs a) {
    constexpr int NX = S::NX, W = NX + NX * NX;
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x;
    const int st = blockIdx.y;
    if (b >= d.B) return;
    if (!a.active[b]) return;
    const int Bp = d.Bp;
    const int k = d.steps.t[st], kp0 = d.steps.kp[st], kp1 = d.steps.kp[st + 1];
    double* out = a.kpd + (size_t)st * W * Bp;
    const double* src = a.kpd + (size_t)(d.steps.n + kp0) * W * Bp;
    NOUNR for (int e = 0; e < W; e++) {
        double v = AT(src, e, b);
        NOUNR for (int j = 1; j < kp1 - kp0; j++) v += AT(src, (size_t)j * W + e, b);
        AT(out, e, b) = v;
    }
    if (d.limits_set) {  // limit terms (System.cpp:121-142), once per step, as stage_derivs_rows adds them for a lone keypoint
        const double* X = a.X[a.cur[b]];
        NOUNR for (int i = 0; i < NX; i++) {
            if (d.lw[i] != 0) {
                const double xi = AT(X, k * NX + i, b);
                double qv = 0, L = 0;
                if (xi > d.smax[i]) { qv = d.smax[i] - xi; L = d.penalty; }
                else if (xi < d.smin[i]) { qv = d.smin[i] - xi; L = d.penalty; }
                AT(out, i, b) += -L * qv;
                AT(out, NX + i * NX + i, b) += (L != 0.0) ? d.pen_xx : 0.0;
            }
        }
    }
}

// Backward Riccati sweep (ILQRRecursive.cpp:68-97): writes K_k, d_k for k = T-2..0.  Needs k_kp_derivs first.
//
// One lane per instance, the reference's operation order (dense products, partial-pivot LU as Eigen's inverse()).  The matrices of a step
// -- 1500 doubles for n_x = 15 against the 256 a lane's whole register file holds -- live in an EXPLICIT workspace in global memory
// (a.ws, entry e of instance b at ws[e Bp + b]: coalesced across the lanes of a wave), walked by plain loops: 60 VGPRs, no scratch, no
// compiler-managed private segment.  (As local arrays of a fully unrolled kernel they made 512-VGPR code objects with up to 7 KB of scratch per
// lane, and in round 1 one of them -- then still with the keypoint code inlined -- ended in a memory aperture violation: DESIGN.md 5.5.)
// The stage derivatives come from k_kp_derivs at the keypoint steps (FK, the quaternion log map, frames, dead zones and J'QJ stay out of
// the sweep) and are the limit terms elsewhere; the second limit set on top of either.
template <class S>
constexpr int backward_ws_doubles() {
    return 3 * S::NX * S::NX + 5 * S::NU * S::NX + 3 * S::NU * S::NU + 4 * S::NX + 2 * S::NU;
}
int backward_ws_entries(int kind, int nd) {
    int n = 0;
    SysAll::dispatch(kind, nd, [&](auto s) { n = backward_ws_doubles<decltype(s)>(); });
    return n;
}

// O = ObsArgs, the OBS form: the slot obd[k] of k_obs_derivs is added to the position block of l_x, l_xx behind the keypoint or limit terms.
template <class S, bool AL, class... O>
__global__ __launch_bounds__(64) void k_backward(Bufs a, O... o) {
    constexpr int NX = S::NX, NU = S::NU, ND = S::ND, TM = S::TM;
    constexpr bool OBS = sizeof...(O) != 0;
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= d.B) return;
    if (!a.active[b]) return;
    const int Bp = d.Bp, T = d.T;
    const int cur = a.cur[b];
    const double* X = a.X[cur];
    const double* U = a.U[cur];
    // workspace views
    double* const w = a.ws + b;
    constexpr int oP = 0, op = oP + NX * NX, oQxx = op + NX, oQx = oQxx + NX * NX, oAtP = oQx + NX, oBtP = oAtP + NX * NX, oQux = oBtP + NU * NX,
                  oQxu = oQux + NU * NX, oK = oQxu + NX * NU, oKtQ = oK + NU * NX, oQuu = oKtQ + NX * NU, oMr = oQuu + NU * NU, oQi = oMr + NU * NU,
                  oQu = oQi + NU * NU, odk = oQu + NU, obc = odk + NU, ox = obc + NX, oEnd = ox + NX;
    static_assert(oEnd == backward_ws_doubles<S>(), "workspace layout");
#define WS(o, i, j, C) w[(size_t)((o) + (i) * (C) + (j)) * Bp]
#define WV(o, i) w[(size_t)((o) + (i)) * Bp]
    // l_xx -> matrix at oM, l_x -> vector at oV for the state at ox (statement for statement stage_derivs / lim2_derivs of ilqr_step.hpp)
    auto stage_to_ws = [&](int kpi_, int k_, int oM, int oV) {
        if (kpi_ >= 0) {
            const double* src = a.kpd + (size_t)kpi_ * (NX + NX * NX) * Bp;
            NOUNR for (int i = 0; i < NX; i++) {
                WV(oV, i) = AT(src, i, b);
                NOUNR for (int j = 0; j < NX; j++) WS(oM, i, j, NX) = AT(src, NX + i * NX + j, b);
            }
        } else {
            NOUNR for (int i = 0; i < NX; i++) {
                double lxi = 0, lxxi = 0;
                NOUNR for (int j = 0; j < NX; j++) WS(oM, i, j, NX) = 0;
                if (d.limits_set && d.lw[i] != 0) {
                    const double xi = WV(ox, i);
                    double qv = 0, L = 0;
                    if (xi > d.smax[i]) { qv = d.smax[i] - xi; L = d.penalty; }
                    else if (xi < d.smin[i]) { qv = d.smin[i] - xi; L = d.penalty; }
                    lxi += -L * qv;
                    lxxi += (L != 0.0) ? d.pen_xx : 0.0;
                }
                WV(oV, i) = lxi;
                WS(oM, i, i, NX) = lxxi;
            }
        }
        if constexpr (OBS) {
            const double* src = obs_slot(o..., k_, Bp);
            NOUNR for (int i = 0; i < DOF; i++) {
                WV(oV, i) += AT(src, OBS_LX + i, b);
                NOUNR for (int j = 0; j < DOF; j++) WS(oM, i, j, NX) += AT(src, OBS_LXX + (i <= j ? obs_tri(i, j) : obs_tri(j, i)), b);
            }
        }
        if (d.lim2) {
            NOUNR for (int i = 0; i < NX; i++) {
                if (d.lw2[i] != 0) {
                    const double xi = WV(ox, i);
                    double qv = 0, L = 0;
                    if (xi > d.smax2[i]) { qv = d.smax2[i] - xi; L = d.penalty2; }
                    else if (xi < d.smin2[i]) { qv = d.smin2[i] - xi; L = d.penalty2; }
                    WV(oV, i) += -L * qv;
                    WS(oM, i, i, NX) += (L != 0.0) ? d.pen_xx2 : 0.0;
                }
            }
        }
    };
    auto is_v = [](int i) { return ND == 2 && i >= DOF && i < 2 * DOF; };

    int kpi = d.steps.n - 1;  // step table walk: the kpd slot of a step holds the sum over its keypoints (k_kp_sum)
    NOUNR for (int i = 0; i < NX; i++) WV(ox, i) = AT(X, (T - 1) * NX + i, b);
    {
        const bool iskp = (kpi >= 0 && d.steps.t[kpi] == T - 1);
        stage_to_ws(iskp ? kpi : -1, T - 1, oP, op);
        if (iskp) kpi--;
    }
    for (int k = T - 2; k >= 0; k--) {
        NOUNR for (int i = 0; i < NX; i++) WV(ox, i) = AT(X, k * NX + i, b);
        const double* u = U + (size_t)k * NU * Bp + b;  // u_i = u[i Bp]
        const double dts = TM ? u[(size_t)(NU - 1) * Bp] : 0.0;
        const double dt = TM ? dts * dts : d.dt;
        const double hdt2 = dt * dt / 2;
        // last column of B for time systems (PosOrnTimePlannerSys.cpp:161-162,176)
        if (TM) {
            if (ND == 1) {
                NOUNR for (int i = 0; i < DOF; i++) WV(obc, i) = 2 * dts * u[(size_t)i * Bp];
            } else {
                NOUNR for (int i = 0; i < DOF; i++) {
                    const double ui = u[(size_t)i * Bp];
                    double dqn = WV(ox, DOF + i) + dt * ui;  // velocity AFTER the step
                    WV(obc, i) = 2 * dts * dqn + 2 * dts * dts * dts * ui;
                    WV(obc, DOF + i) = 2 * dts * ui;
                }
            }
            WV(obc, NX - 1) = 2 * dts;
        }
        {   // l_xx, l_x of the stage go straight into the Qxx / Qx slots (Qxx = l_xx + A'PA below)
            const bool iskp = (kpi >= 0 && d.steps.t[kpi] == k);
            stage_to_ws(iskp ? kpi : -1, k, oQxx, oQx);
            if (iskp) kpi--;
        }
        // BtP = B^T P (NU x NX), AtP = A^T P (NX x NX)
        NOUNR for (int i = 0; i < DOF; i++)
            NOUNR for (int j = 0; j < NX; j++)
                WS(oBtP, i, j, NX) = (ND == 1) ? dt * WS(oP, i, j, NX) : hdt2 * WS(oP, i, j, NX) + dt * WS(oP, DOF + i, j, NX);
        if (TM) {
            NOUNR for (int j = 0; j < NX; j++) {
                double s = 0;
                NOUNR for (int l = 0; l < NX; l++) s += WV(obc, l) * WS(oP, l, j, NX);
                WS(oBtP, NU - 1, j, NX) = s;
            }
        }
        NOUNR for (int i = 0; i < NX; i++)
            NOUNR for (int j = 0; j < NX; j++)
                WS(oAtP, i, j, NX) = is_v(i) ? dt * WS(oP, i - DOF, j, NX) + WS(oP, i, j, NX) : WS(oP, i, j, NX);
        // Qux = BtP A ; Quu = R + BtP B ; Qxx = lxx + AtP A ; Qxu = AtP B ; Qu = R u + B^T p ; Qx = lx + A^T p
        NOUNR for (int i = 0; i < NU; i++) {
            NOUNR for (int j = 0; j < NX; j++)
                WS(oQux, i, j, NX) = is_v(j) ? WS(oBtP, i, j - DOF, NX) * dt + WS(oBtP, i, j, NX) : WS(oBtP, i, j, NX);
            NOUNR for (int j = 0; j < DOF; j++)
                WS(oQuu, i, j, NU) = (ND == 1) ? WS(oBtP, i, j, NX) * dt : WS(oBtP, i, j, NX) * hdt2 + WS(oBtP, i, DOF + j, NX) * dt;
            if (TM) {
                double s = 0;
                NOUNR for (int l = 0; l < NX; l++) s += WS(oBtP, i, l, NX) * WV(obc, l);
                WS(oQuu, i, NU - 1, NU) = s;
            }
            WS(oQuu, i, i, NU) = d.R_diag[i] + WS(oQuu, i, i, NU);
        }
        NOUNR for (int i = 0; i < NX; i++) {
            NOUNR for (int j = 0; j < NX; j++) {
                double v = is_v(j) ? WS(oAtP, i, j - DOF, NX) * dt + WS(oAtP, i, j, NX) : WS(oAtP, i, j, NX);
                WS(oQxx, i, j, NX) = WS(oQxx, i, j, NX) + v;
            }
            NOUNR for (int j = 0; j < DOF; j++)
                WS(oQxu, i, j, NU) = (ND == 1) ? WS(oAtP, i, j, NX) * dt : WS(oAtP, i, j, NX) * hdt2 + WS(oAtP, i, DOF + j, NX) * dt;
            if (TM) {
                double s = 0;
                NOUNR for (int l = 0; l < NX; l++) s += WS(oAtP, i, l, NX) * WV(obc, l);
                WS(oQxu, i, NU - 1, NU) = s;
            }
        }
        NOUNR for (int i = 0; i < DOF; i++) {
            double v = (ND == 1) ? dt * WV(op, i) : hdt2 * WV(op, i) + dt * WV(op, DOF + i);
            WV(oQu, i) = d.R_diag[i] * u[(size_t)i * Bp] + v;
        }
        if (TM) {
            double s = 0;
            NOUNR for (int l = 0; l < NX; l++) s += WV(obc, l) * WV(op, l);
            WV(oQu, NU - 1) = d.R_diag[NU - 1] * u[(size_t)(NU - 1) * Bp] + s;
        }
        NOUNR for (int i = 0; i < NX; i++) {
            double v = is_v(i) ? dt * WV(op, i - DOF) + WV(op, i) : WV(op, i);
            WV(oQx, i) = WV(oQx, i) + v;
        }
        if (AL) {  // AL-ILQR.cpp:110-134: c_u' I c_x etc., lambda + I c
            const int ns = NX + NU;
            for (int r = 0; r < a.m; r++) {
                const double* Ar = a.conA + ((size_t)(a.per_step ? k : 0) * a.m + r) * ns;
                const double Ik = AT(a.Is, k * a.m + r, b);
                const double lam = AT(a.lambda, k * a.m + r, b);
                double g = 0;  // con_g (ilqr_step.hpp): A [x;u] - b, same order
                NOUNR for (int i = 0; i < NX; i++) g += Ar[i] * WV(ox, i);
                NOUNR for (int i = 0; i < NU; i++) g += Ar[NX + i] * u[(size_t)i * Bp];
                g = g - a.conb[(size_t)(a.per_step ? k : 0) * a.m + r];
                const double wv = lam + Ik * g;
                NOUNR for (int i = 0; i < NU; i++) {
                    const double au = Ar[NX + i];
                    NOUNR for (int j = 0; j < NX; j++) WS(oQux, i, j, NX) += au * Ik * Ar[j];
                    NOUNR for (int j = 0; j < NU; j++) WS(oQuu, i, j, NU) += au * Ik * Ar[NX + j];
                    WV(oQu, i) += au * wv;
                }
                NOUNR for (int i = 0; i < NX; i++) {
                    const double ax = Ar[i];
                    NOUNR for (int j = 0; j < NX; j++) WS(oQxx, i, j, NX) += ax * Ik * Ar[j];
                    NOUNR for (int j = 0; j < NU; j++) WS(oQxu, i, j, NU) += ax * Ik * Ar[NX + j];
                    WV(oQx, i) += ax * wv;
                }
            }
        }
        // Quu_inv = -(Quu + reg I)^-1 ; K = Quu_inv Qux ; d = Quu_inv Qu.  Inverse: Eigen's MatrixXd::inverse() = PartialPivLU + solve against
        // the identity (the algorithm of inverse_lu in ilqr_step.hpp, on the workspace)
        NOUNR for (int i = 0; i < NU; i++)
            NOUNR for (int j = 0; j < NU; j++) WS(oMr, i, j, NU) = WS(oQuu, i, j, NU) + ((i == j) ? d.reg : 0.0);
        {
            unsigned long long piv = 0;  // row permutation, 4 bits per row
            NOUNR for (int i = 0; i < NU; i++) piv |= (unsigned long long)i << (4 * i);
            NOUNR for (int kk = 0; kk < NU; kk++) {
                double best = fabs(WS(oMr, kk, kk, NU));
                int r = kk;
                NOUNR for (int i = kk + 1; i < NU; i++) {
                    const double v = fabs(WS(oMr, i, kk, NU));
                    if (v > best) { best = v; r = i; }
                }
                if (r != kk) {
                    NOUNR for (int j = 0; j < NU; j++) {
                        const double t0 = WS(oMr, kk, j, NU), t1 = WS(oMr, r, j, NU);
                        WS(oMr, kk, j, NU) = t1;
                        WS(oMr, r, j, NU) = t0;
                    }
                    const unsigned long long p0 = (piv >> (4 * kk)) & 15ull, p1 = (piv >> (4 * r)) & 15ull;
                    piv = (piv & ~((15ull << (4 * kk)) | (15ull << (4 * r)))) | (p1 << (4 * kk)) | (p0 << (4 * r));
                }
                const double pv = WS(oMr, kk, kk, NU);
                NOUNR for (int i = kk + 1; i < NU; i++) {
                    WS(oMr, i, kk, NU) /= pv;
                    const double f = WS(oMr, i, kk, NU);
                    NOUNR for (int j = kk + 1; j < NU; j++) WS(oMr, i, j, NU) -= f * WS(oMr, kk, j, NU);
                }
            }
            NOUNR for (int c = 0; c < NU; c++) {
                NOUNR for (int i = 0; i < NU; i++) {
                    double s = ((int)((piv >> (4 * i)) & 15ull) == c) ? 1.0 : 0.0;
                    NOUNR for (int j = 0; j < i; j++) s -= WS(oMr, i, j, NU) * WS(oQi, j, c, NU);
                    WS(oQi, i, c, NU) = s;
                }
                NOUNR for (int i = NU - 1; i >= 0; i--) {
                    double s = WS(oQi, i, c, NU);
                    NOUNR for (int j = i + 1; j < NU; j++) s -= WS(oMr, i, j, NU) * WS(oQi, j, c, NU);
                    WS(oQi, i, c, NU) = s / WS(oMr, i, i, NU);
                }
            }
        }
        double* const Krec = KD_REC(a.KD, Bp, NU * kd_rowp(NX), k, b);
        NOUNR for (int i = 0; i < NU; i++) {
            NOUNR for (int j = 0; j < NX; j++) {
                double s = 0;
                NOUNR for (int l = 0; l < NU; l++) s += (-1 * WS(oQi, i, l, NU)) * WS(oQux, l, j, NX);
                WS(oK, i, j, NX) = s;
                Krec[i * kd_rowp(NX) + j] = s;
            }
            double s = 0;
            NOUNR for (int l = 0; l < NU; l++) s += (-1 * WS(oQi, i, l, NU)) * WV(oQu, l);
            WV(odk, i) = s;
            Krec[i * kd_rowp(NX) + NX] = s;
        }
        // P = Qxx + K'QuuK + K'Qux + QxuK ; p = Qx + K'Quu d + K'Qu + Qxu d   (un-regularised Quu)
        NOUNR for (int i = 0; i < NX; i++)
            NOUNR for (int j = 0; j < NU; j++) {
                double s = 0;
                NOUNR for (int l = 0; l < NU; l++) s += WS(oK, l, i, NX) * WS(oQuu, l, j, NU);
                WS(oKtQ, i, j, NU) = s;
            }
        NOUNR for (int i = 0; i < NX; i++) {
            NOUNR for (int j = 0; j < NX; j++) {
                double t1 = 0, t2 = 0, t3 = 0;
                NOUNR for (int l = 0; l < NU; l++) {
                    t1 += WS(oKtQ, i, l, NU) * WS(oK, l, j, NX);
                    t2 += WS(oK, l, i, NX) * WS(oQux, l, j, NX);
                    t3 += WS(oQxu, i, l, NU) * WS(oK, l, j, NX);
                }
                WS(oP, i, j, NX) = ((WS(oQxx, i, j, NX) + t1) + t2) + t3;
            }
            double v1 = 0, v2 = 0, v3 = 0;
            NOUNR for (int l = 0; l < NU; l++) {
                v1 += WS(oKtQ, i, l, NU) * WV(odk, l);
                v2 += WS(oK, l, i, NX) * WV(oQu, l);
                v3 += WS(oQxu, i, l, NU) * WV(odk, l);
            }
            WV(op, i) = ((WV(oQx, i) + v1) + v2) + v3;
        }
    }
#undef WS
#undef WV
}

// ---- obstacle terms (ilqr_obstacle.hpp)

// obd[k] = c_obs | l_x | upper triangle of l_xx of step k of every instance's current trajectory, one lane per (instance, step): lanes along the
// batch, so every load is a whole run of a [row][Bp] row of X[cur] and every store a whole run of a row of the slot; the geometry is read at
// wave-uniform addresses.  Runs where k_kp_derivs runs, before every sweep (all = 0: the instances the sweep visits), and for the query call
// (all = 1).  The generic path applies a line search's winner inside its forward pass, so X[cur] is the accepted trajectory.
__global__ __launch_bounds__(64) void k_obs_derivs(Bufs a, ObsArgs o, int nx, int k0, int all) {
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x;
    const int k = k0 + (int)blockIdx.y;
    if (b >= d.B) return;
    if (!all && !a.active[b]) return;
    const size_t Bps = (size_t)d.Bp;
    const double* x = a.X[a.cur[b]] + (size_t)k * (size_t)nx * Bps + (size_t)b;
    double lx[7], lxx[28];
    const double c = obs_state<true>(*o.geom, o.obs + (size_t)(b / o.traj_per_set) * (size_t)o.n_obs * 4, o.n_obs, o.margin, o.weight,
                                     [&](int j) { return x[(size_t)j * Bps]; }, lx, lxx);
    double* out = o.obd + (size_t)k * OBS_W * Bps + (size_t)b;
    out[0] = c;
    UNR for (int i = 0; i < 7; i++) out[(size_t)(OBS_LX + i) * Bps] = lx[i];
    UNR for (int e = 0; e < 28; e++) out[(size_t)(OBS_LXX + e) * Bps] = lxx[e];
}

// ilqr_problem_obstacle_terms: the slots in the natural layout on the user's joints; l_xx mirrored from its upper triangle
__global__ __launch_bounds__(256) void k_obs_query(const double* __restrict__ obd, int B, int Bp, int T, int dof, double* __restrict__ cost,
                                                   double* __restrict__ lx, double* __restrict__ lxx) {
    const int b = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (b >= B) return;
    const double* s = obd + (size_t)k * OBS_W * (size_t)Bp + (size_t)b;
    const size_t e = (size_t)b * (size_t)T + (size_t)k;
    if (cost) cost[e] = s[0];
    for (int i = 0; i < dof; i++) {
        if (lx) lx[e * dof + i] = s[(size_t)(OBS_LX + i) * Bp];
        if (lxx)
            for (int j = 0; j < dof; j++) lxx[(e * dof + i) * dof + j] = s[(size_t)(OBS_LXX + (i <= j ? obs_tri(i, j) : obs_tri(j, i))) * Bp];
    }
}

// ------------------------------------------------------------------------------------------------ gather / scatter

// natural [B][rows] (host/ABI layout) <-> device [rows][Bp]
__global__ void k_to_soa(const double* __restrict__ src, double* __restrict__ dst, int B, int Bp, int rows) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (b < B) dst[(size_t)r * Bp + b] = src[(size_t)b * rows + r];
}
__global__ void k_from_soa(const double* __restrict__ src, double* __restrict__ dst, int B, int Bp, int rows) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (b < B) dst[(size_t)b * rows + r] = src[(size_t)r * Bp + b];
}
// same, selecting each instance's current trajectory buffer
__global__ void k_from_soa_cur(const double* __restrict__ s0, const double* __restrict__ s1, const int* __restrict__ cur,
                               double* __restrict__ dst, int B, int Bp, int rows) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (b < B) dst[(size_t)b * rows + r] = (cur[b] ? s1 : s0)[(size_t)r * Bp + b];
}
// returned ds are scaled by the accepted alpha (ILQRRecursive.cpp:128,144,162)
__global__ void k_from_soa_scaled(const double* __restrict__ src, const double* __restrict__ alpha, const int* __restrict__ iters,
                                  double* __restrict__ dst, int B, int Bp, int rows) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (b < B) dst[(size_t)b * rows + r] = (iters[b] > 0 ? alpha[b] : 1.0) * src[(size_t)r * Bp + b];
}

// gains in the reference's layout: K[B][T-1][NU][NX], d[B][T-1][NU] scaled by the accepted alpha (ILQRRecursive.cpp:128,144,162)
__global__ void k_get_gains(const double* __restrict__ kd, int sym, const double* __restrict__ alpha, const int* __restrict__ iters,
                            double* __restrict__ K_out, double* __restrict__ d_out, int B, int Bp, int T1, int nu, int nx) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (b >= B) return;
    const int rowp = kd_rowp(nx), rs = kd_rs(sym, nu, rowp);  // (sym: the packed symmetric record of the uniform-R single-integrator sweep)
    const double* rec = KD_REC(kd, Bp, rs, k, b);
    const double sc = (iters[b] > 0) ? alpha[b] : 1.0;
    for (int i = 0; i < nu; i++) {
        if (K_out)
            for (int j = 0; j < nx; j++) K_out[(((size_t)b * T1 + k) * nu + i) * nx + j] = rec[kd_off(sym, rowp, i, j)];
        if (d_out) d_out[((size_t)b * T1 + k) * nu + i] = sc * rec[kd_off(sym, rowp, i, nx)];
    }
}

// Receding-horizon warm start: the next solve starts from the accepted plan shifted by `shift` timesteps --
// U0[k] = U[min(k + shift, T-2)], q0 (dq0) = the joint part of x_{shift}.  One lane per (instance, timestep).
__global__ void k_warm_start(Bufs a, double* __restrict__ U0, double* __restrict__ q0, double* __restrict__ dq0, int shift, int nx, int nu, int nd) {
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (b >= d.B) return;
    const int Bp = d.Bp, T = d.T;
    const int cur = a.cur[b];
    const int ks = (k + shift < T - 1) ? k + shift : T - 2;
    for (int i = 0; i < nu; i++) AT(U0, k * nu + i, b) = AT(a.U[cur], ks * nu + i, b);
    if (k == 0 && shift > 0) {
        const int kx = shift < T ? shift : T - 1;
        for (int i = 0; i < DOF; i++) {
            AT(q0, i, b) = AT(a.X[cur], kx * nx + i, b);
            if (nd == 2) AT(dq0, i, b) = AT(a.X[cur], kx * nx + DOF + i, b);
        }
    }
}

// Tracking law of the tutorials (POS_ORN_SYS.ipynb cell 7): u = ubar_k + K_k (x - xbar_k) [+ alpha d_k] for a measured state
// per instance; natural layouts x_meas[B][NX], u_out[B][NU].  One lane per instance.
__global__ void k_track(Bufs a, const double* __restrict__ x_meas, int k, int with_ff, double* __restrict__ u_out, int nx, int nu) {
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= d.B) return;
    const int Bp = d.Bp;
    const int cur = a.cur[b];
    const int sym = a.kd_sym, rowp = kd_rowp(nx), rs = kd_rs(sym, nu, rowp);
    const double* rec = KD_REC(a.KD, Bp, rs, k, b);
    const double sc = (a.iters[b] > 0) ? a.alpha[b] : 1.0;
    for (int i = 0; i < nu; i++) {
        double s = AT(a.U[cur], k * nu + i, b);
        for (int j = 0; j < nx; j++) s += rec[kd_off(sym, rowp, i, j)] * (x_meas[(size_t)b * nx + j] - AT(a.X[cur], k * nx + j, b));
        if (with_ff) s += sc * rec[kd_off(sym, rowp, i, nx)];
        u_out[(size_t)b * nu + i] = s;
    }
}

// ---- chains of fewer than 7 joints (ilqr_dofmap.hpp): the conversions above with the per-step vectors widened / narrowed through their map.
// The map is a kernel argument; row r of a block is one vector entry, so its map lookup is uniform over the block (a scalar load).

// natural [B][outer][m.n_user] -> device [outer][m.n_dev][Bp]; padded entries are written as 0
__global__ void k_to_soa_map(const double* __restrict__ src, double* __restrict__ dst, int B, int Bp, IndexMap m) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y, o = r / m.n_dev, i = m.usr[r - o * m.n_dev];
    const size_t rows_user = (size_t)(gridDim.y / m.n_dev) * m.n_user;
    if (b < B) dst[(size_t)r * Bp + b] = i < 0 ? 0.0 : src[(size_t)b * rows_user + (size_t)o * m.n_user + i];
}
// device [outer][m.n_dev][Bp] (each instance's current buffer) -> natural [B][outer][m.n_user]
__global__ void k_from_soa_cur_map(const double* __restrict__ s0, const double* __restrict__ s1, const int* __restrict__ cur,
                                   double* __restrict__ dst, int B, int Bp, IndexMap m) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y, o = r / m.n_user, j = m.dev[r - o * m.n_user];
    const size_t rows_user = gridDim.y;
    if (b < B) dst[(size_t)b * rows_user + r] = (cur && cur[b] ? s1 : s0)[((size_t)o * m.n_dev + j) * Bp + b];
}
// k_get_gains on the user's rows (controls) and columns (states)
__global__ void k_get_gains_map(const double* __restrict__ kd, int sym, const double* __restrict__ alpha, const int* __restrict__ iters,
                                double* __restrict__ K_out, double* __restrict__ d_out, int B, int Bp, int T1, IndexMap x, IndexMap u) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (b >= B) return;
    const int nx = x.n_dev, rowp = kd_rowp(nx), rs = kd_rs(sym, u.n_dev, rowp);
    const double* rec = KD_REC(kd, Bp, rs, k, b);
    const double sc = (iters[b] > 0) ? alpha[b] : 1.0;
    const int nu = u.n_user, nxu = x.n_user;
    for (int i = 0; i < nu; i++) {
        const int id = u.dev[i];
        if (K_out)
            for (int j = 0; j < nxu; j++) K_out[(((size_t)b * T1 + k) * nu + i) * nxu + j] = rec[kd_off(sym, rowp, id, x.dev[j])];
        if (d_out) d_out[((size_t)b * T1 + k) * nu + i] = sc * rec[kd_off(sym, rowp, id, nx)];
    }
}
// k_track on the user's layouts x_meas[B][x.n_user], u_out[B][u.n_user].  The padded state entries of the device trajectory are 0, as the
// padding of a measured state would be: the terms left out add exactly 0.
__global__ void k_track_map(Bufs a, const double* __restrict__ x_meas, int k, int with_ff, double* __restrict__ u_out, IndexMap x, IndexMap u) {
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= d.B) return;
    const int Bp = d.Bp, nx = x.n_dev, nu = u.n_dev;
    const int cur = a.cur[b];
    const int sym = a.kd_sym, rowp = kd_rowp(nx), rs = kd_rs(sym, nu, rowp);
    const double* rec = KD_REC(a.KD, Bp, rs, k, b);
    const double sc = (a.iters[b] > 0) ? a.alpha[b] : 1.0;
    for (int i = 0; i < u.n_user; i++) {
        const int id = u.dev[i];
        double s = AT(a.U[cur], k * nu + id, b);
        for (int j = 0; j < x.n_user; j++) {
            const int jd = x.dev[j];
            s += rec[kd_off(sym, rowp, id, jd)] * (x_meas[(size_t)b * x.n_user + j] - AT(a.X[cur], k * nx + jd, b));
        }
        if (with_ff) s += sc * rec[kd_off(sym, rowp, id, nx)];
        u_out[(size_t)b * u.n_user + i] = s;
    }
}

// Closed loop of the tracking law (ilqr_closed_loop.hpp): S executions per instance from the caller's start states under the caller's
// disturbances, one lane per (instance, sample), k_init_rollout's loop with the control of k_track in place of U0.  Natural layouts on the
// user's dimensions (ClArgs), addressed with 32-bit element offsets (checked by the host).  MAP: a chain of fewer than 7 joints -- device
// entry i is the user's mx.usr[i]; padded entries start on the plan (0), get no disturbance and keep the plan's control.  CON: judge the
// constraint rows (ilqr_problem_closed_loop_report_con; c.con_max is given).  A template argument like the cooperative kernel's FF: as a
// run-time branch it pushed the 2nd-order instantiations, which sit at the register ceiling, into scratch.
template <class S, bool MAP, bool CON>
__global__ __launch_bounds__(64) void k_closed_loop(Bufs a, ClArgs c, IndexMap mx, IndexMap mu) {
    constexpr int NX = S::NX, NU = S::NU;
    const DevDesc& d = *a.desc;
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= d.B * c.S) return;
    const int b = g / c.S;
    const int Bp = d.Bp, T = d.T, cur = a.cur[b];
    const int nxu = MAP ? mx.n_user : NX, nuu = MAP ? mu.n_user : NU;
    const int sym = a.kd_sym, rs = kd_rs(sym, NU, kd_rowp(NX));
    const double sc = (a.iters[b] > 0) ? a.alpha[b] : 1.0;
    const double* Xb = a.X[cur] + b;  // entry `row` of the plan: Xb[row * Bp]
    const double* Ub = a.U[cur] + b;
    double x[NX], u[NU], xn[NX];
    UNR for (int i = 0; i < NX; i++) {
        const int iu = MAP ? mx.usr[i] : i;
        x[i] = (c.x0 && iu >= 0) ? c.x0[g * nxu + iu] : Xb[(size_t)i * Bp];
    }
    const unsigned gb = c.b_off + (unsigned)b, gs = c.s_off + (unsigned)(g - b * c.S);   // the counter of this lane's draws
    if (c.noise) {
        double nz[NX];
        const unsigned on = noise_draw<NX, MAP, true>(c.seed, gb, gs, NOISE_STEP_START, c.sigma_x0, nxu, mx.usr, nz);
        UNR for (int i = 0; i < NX; i++) if ((on >> i) & 1u) x[i] += nz[i];
    }
    double lim = 0, kpc = 0;
    ClCon con;
    int st = 0;  // step table walk, as in k_init_rollout
    for (int k = 0; k < T - 1; k++) {
        if (c.X) {
            UNR for (int i = 0; i < NX; i++) { const int iu = MAP ? mx.usr[i] : i; if (iu >= 0) c.X[(g * T + k) * nxu + iu] = x[i]; }
        }
        cl_control<S>(KD_REC(a.KD, Bp, rs, k, b), sym, c.with_ff, Xb + (size_t)k * NX * Bp, Ub + (size_t)k * NU * Bp, Bp, sc, x, u);
        if (MAP) { UNR for (int i = 0; i < NU; i++) if (mu.usr[i] < 0) u[i] = Ub[((size_t)k * NU + i) * Bp]; }
        if (c.U) {
            UNR for (int i = 0; i < NU; i++) { const int iu = MAP ? mu.usr[i] : i; if (iu >= 0) c.U[(g * (T - 1) + k) * nuu + iu] = u[i]; }
        }
        if constexpr (CON) cl_con<S>(a, c.con_tol, k, x, u, con);  // before FK: x and u are live here anyway
        lim += cl_limits<S>(d, x);
        if (st < d.steps.n && d.steps.t[st] == k) {
            if (c.kpx) cl_store_kpx<NX, NU>(c, d, st, g, x);  // uniform: only the report asks
            kpc = cl_kp_terms<S>(d, a, b, st, x, u, kpc);
            st++;
        }
        // the draw of this step: behind the keypoint terms, so that it is not live across FK; it depends on no state and fills dyn_step's latency
        double nz[NX];
        unsigned on = 0;
        if (c.noise) on = noise_draw<NX, MAP, true>(c.seed, gb, gs, (unsigned)k, c.sigma_w, nxu, mx.usr, nz);
        dyn_step<S>(d, x, u, xn);
        if (c.noise) cl_disturb<NX, MAP>(c, g, k, T, nxu, mx.usr, on, nz, true, xn);
        else if (c.w) {
            UNR for (int i = 0; i < NX; i++) { const int iu = MAP ? mx.usr[i] : i; if (iu >= 0) xn[i] += c.w[(g * (T - 1) + k) * nxu + iu]; }
        }
        UNR for (int i = 0; i < NX; i++) x[i] = xn[i];
    }
    if (c.X) {
        UNR for (int i = 0; i < NX; i++) { const int iu = MAP ? mx.usr[i] : i; if (iu >= 0) c.X[(g * T + T - 1) * nxu + iu] = x[i]; }
    }
    lim += cl_limits<S>(d, x);
    if (st < d.steps.n && d.steps.t[st] == T - 1) {
        double zu[NU];
        UNR for (int i = 0; i < NU; i++) zu[i] = 0;
        if (c.kpx) cl_store_kpx<NX, NU>(c, d, st, g, x);
        kpc = cl_kp_terms<S>(d, a, b, st, x, zu, kpc);
    }
    if (c.lim_cost) c.lim_cost[g] = lim;
    if constexpr (CON) cl_con_store(c, g, con);
    c.cost[g] = lim + kpc;
}

// ---- ilqr_problem_closed_loop_report: what the executions did at the keypoints and against the limits (definitions: include/ilqr_hip.h)

ILQR_DEV double cl_norm3(const double* e) { return sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]); }

// The five errors of every (pair g = b * S + s, keypoint): one lane per (g, keypoint), g fastest (blockIdx.y = keypoint), so the reads of
// kpx -- [steps.n][n_x + n_u][B * S], the states either rollout stored -- coalesce.  The residual is kp_cost's: fx_of through the keypoint's
// frame, then kp_diff (a joint keypoint: target - x); no dead zone.  Device layout: the padded entries of a chain of fewer than 7 joints
// are 0 in the state and in the target and contribute 0.  Serves both rollouts, so their reports agree by construction.
template <class S>
__global__ __launch_bounds__(64) void k_closed_loop_kp_err(Bufs a, int n_samples, const double* __restrict__ kpx, double* __restrict__ kp_err) {
    constexpr int NX = S::NX, NU = S::NU;
    const DevDesc& d = *a.desc;
    const size_t BS = (size_t)d.B * n_samples;
    const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
    const int kpi = blockIdx.y, n_kp = d.steps.kp[d.steps.n];
    if (g >= BS || kpi >= n_kp) return;
    const int b = (int)(g / (size_t)n_samples), Bp = d.Bp;
    int st = 0;  // the step-table entry that holds keypoint kpi
    while (st + 1 < d.steps.n && d.steps.kp[st + 1] <= kpi) st++;
    const double* o = kpx + (size_t)st * (NX + NU) * BS + g;
    double x[NX], tg[S::NF];
    UNR for (int i = 0; i < NX; i++) x[i] = o[(size_t)i * BS];
    UNR for (int i = 0; i < S::NF; i++) tg[i] = AT(a.kp_tg, kpi * S::NF + i, b);
    double err[ILQR_KP_ERR] = {0, 0, 0, 0, 0};
    if (!S::JOINT && S::ND == 1 && d.kp_joint[kpi]) {  // joint-space keypoint of a hybrid sequence: e = target - x (kp_cost)
        double ss = 0;
        UNR for (int i = 0; i < DOF; i++) ss += (tg[i] - x[i]) * (tg[i] - x[i]);
        err[ILQR_KP_ERR_POS] = sqrt(ss);
        if (S::TM) err[ILQR_KP_ERR_TIME] = fabs(tg[NX - 1] - x[NX - 1]);
    } else {
        double fxv[S::NF], e[S::NQ];
        fx_of<S, false>(d, x, fxv, nullptr, kpi);
        kp_diff<S>(tg, fxv, e);
        if (S::JOINT) {
            double ss = 0;
            UNR for (int i = 0; i < DOF; i++) ss += e[i] * e[i];
            err[ILQR_KP_ERR_POS] = sqrt(ss);
        } else {
            err[ILQR_KP_ERR_POS] = cl_norm3(e);
            err[ILQR_KP_ERR_ORN] = cl_norm3(e + 3);
            if (S::ND == 2) {
                err[ILQR_KP_ERR_VEL] = cl_norm3(e + 6);
                err[ILQR_KP_ERR_ANGVEL] = cl_norm3(e + 9);
            }
        }
        if (S::TM) err[ILQR_KP_ERR_TIME] = fabs(e[S::NQ - 1]);
    }
    double* out = kp_err + (g * (size_t)n_kp + kpi) * ILQR_KP_ERR;
    UNR for (int j = 0; j < ILQR_KP_ERR; j++) out[j] = err[j];
}

// an execution with errors err[ILQR_KP_ERR] misses the keypoint whose tolerances are tol[ILQR_KP_ERR]: strict, a negative tolerance is not judged
ILQR_DEV bool cl_kp_miss(const double* err, const double* tol) {
    bool m = false;
    UNR for (int j = 0; j < ILQR_KP_ERR; j++) m = m || (!(tol[j] < 0) && err[j] > tol[j]);
    return m;
}

// kp_stats[b][k] = { mean[5], max[5], n_miss, n_bad } of kp_err[b][0 .. S-1][k]: one lane per (instance, keypoint) over the samples in sample
// order (blockIdx.y = keypoint), like k_closed_loop_stats and for its reason: the sums do not depend on the batch size or on the kernel pin.
__global__ __launch_bounds__(64) void k_closed_loop_kp_stats(const double* __restrict__ kp_err, ilqr_cl_tol tol, int B, int S, int n_kp,
                                                            double* __restrict__ kp_stats) {
    const int b = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y;
    if (b >= B || k >= n_kp) return;
    double sum[ILQR_KP_ERR], hi[ILQR_KP_ERR], tk[ILQR_KP_ERR];
    UNR for (int j = 0; j < ILQR_KP_ERR; j++) { sum[j] = 0; hi[j] = -INFINITY; tk[j] = tol.kp_tol[k][j]; }
    int n = 0, n_miss = 0;
    for (int s = 0; s < S; s++) {
        const double* e = kp_err + (((size_t)b * S + s) * n_kp + k) * ILQR_KP_ERR;
        double v[ILQR_KP_ERR];
        bool good = true;
        UNR for (int j = 0; j < ILQR_KP_ERR; j++) { v[j] = e[j]; good = good && isfinite(v[j]); }
        if (!good) continue;
        n++;
        UNR for (int j = 0; j < ILQR_KP_ERR; j++) { sum[j] += v[j]; hi[j] = v[j] > hi[j] ? v[j] : hi[j]; }
        if (cl_kp_miss(v, tk)) n_miss++;
    }
    double* o = kp_stats + ((size_t)b * n_kp + k) * ILQR_KP_STATS;
    UNR for (int j = 0; j < ILQR_KP_ERR; j++) { o[j] = n ? sum[j] / n : NAN; o[ILQR_KP_ERR + j] = n ? hi[j] : NAN; }
    o[2 * ILQR_KP_ERR] = (double)n_miss;
    o[2 * ILQR_KP_ERR + 1] = (double)(S - n);
}

// outcome[b] = { n_ok, n_miss, n_lim, n_bad }: one lane per instance over its samples
__global__ __launch_bounds__(64) void k_closed_loop_outcome(const double* __restrict__ cost, const double* __restrict__ kp_err,
                                                           const double* __restrict__ lim_cost, ilqr_cl_tol tol, int B, int S, int n_kp,
                                                           double* __restrict__ outcome) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int n_ok = 0, n_miss = 0, n_lim = 0, n_bad = 0;
    for (int s = 0; s < S; s++) {
        const size_t g = (size_t)b * S + s;
        if (!isfinite(cost[g])) { n_bad++; continue; }
        bool miss = false;
        for (int k = 0; k < n_kp; k++) {
            const double* e = kp_err + (g * n_kp + k) * ILQR_KP_ERR;
            double v[ILQR_KP_ERR];
            UNR for (int j = 0; j < ILQR_KP_ERR; j++) v[j] = e[j];
            miss = miss || cl_kp_miss(v, tol.kp_tol[k]);
        }
        const bool lim = lim_cost[g] > tol.lim_tol;
        n_miss += miss ? 1 : 0;
        n_lim += lim ? 1 : 0;
        n_ok += (!miss && !lim) ? 1 : 0;
    }
    double* o = outcome + (size_t)b * ILQR_CL_OUTCOME;
    o[0] = (double)n_ok; o[1] = (double)n_miss; o[2] = (double)n_lim; o[3] = (double)n_bad;
}

// con_stats[b] = { mean con_max, max con_max, mean con_steps, max con_steps, n_con, n_bad } of con_max / con_steps[b][0 .. S-1]: one lane per
// instance over the samples in sample order, like k_closed_loop_stats and for its reason.  A sample is bad if its con_max is not finite.
__global__ __launch_bounds__(64) void k_closed_loop_con_stats(const double* __restrict__ con_max, const double* __restrict__ con_steps,
                                                             double con_tol, int B, int S, double* __restrict__ con_stats) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int n = 0, n_con = 0;
    double sm = 0, hm = -INFINITY, ss = 0, hs = -INFINITY;
    for (int s = 0; s < S; s++) {
        const size_t g = (size_t)b * S + s;
        const double v = con_max[g], q = con_steps[g];
        if (!isfinite(v)) continue;
        n++;
        sm += v; hm = v > hm ? v : hm;
        ss += q; hs = q > hs ? q : hs;
        if (v > con_tol) n_con++;
    }
    double* o = con_stats + (size_t)b * ILQR_CL_CON_STATS;
    o[0] = n ? sm / n : NAN;
    o[1] = n ? hm : NAN;
    o[2] = n ? ss / n : NAN;
    o[3] = n ? hs : NAN;
    o[4] = (double)n_con;
    o[5] = (double)(S - n);
}

// outcome_con[b] = { n_ok, n_miss, n_lim, n_con, n_bad }: k_closed_loop_outcome with the constraint rows as a third way to fail
__global__ __launch_bounds__(64) void k_closed_loop_outcome_con(const double* __restrict__ cost, const double* __restrict__ kp_err,
                                                               const double* __restrict__ lim_cost, const double* __restrict__ con_max,
                                                               ilqr_cl_tol tol, double con_tol, int B, int S, int n_kp,
                                                               double* __restrict__ outcome_con) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int n_ok = 0, n_miss = 0, n_lim = 0, n_con = 0, n_bad = 0;
    for (int s = 0; s < S; s++) {
        const size_t g = (size_t)b * S + s;
        if (!isfinite(cost[g])) { n_bad++; continue; }
        bool miss = false;
        for (int k = 0; k < n_kp; k++) {
            const double* e = kp_err + (g * n_kp + k) * ILQR_KP_ERR;
            double v[ILQR_KP_ERR];
            UNR for (int j = 0; j < ILQR_KP_ERR; j++) v[j] = e[j];
            miss = miss || cl_kp_miss(v, tol.kp_tol[k]);
        }
        const bool lim = lim_cost[g] > tol.lim_tol;
        const double cm = con_max[g];
        const bool con = cm > con_tol || !isfinite(cm);
        n_miss += miss ? 1 : 0;
        n_lim += lim ? 1 : 0;
        n_con += con ? 1 : 0;
        n_ok += (!miss && !lim && !con) ? 1 : 0;
    }
    double* o = outcome_con + (size_t)b * ILQR_CL_OUTCOME_CON;
    o[0] = (double)n_ok; o[1] = (double)n_miss; o[2] = (double)n_lim; o[3] = (double)n_con; o[4] = (double)n_bad;
}

// Per-instance statistics of the closed-loop costs: one lane per instance over cost[b][0 .. S-1] in sample order, in two passes, so the sums do
// not depend on the batch size or on which kernel made the costs.  stats[b] = { mean, unbiased variance, min, max, n_bad }: n_bad counts the
// samples whose cost is not finite, the other four are over the finite ones (variance 0 for a single one, all four NaN for none).
__global__ __launch_bounds__(64) void k_closed_loop_stats(const double* __restrict__ cost, int B, int S, double* __restrict__ stats) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double* cb = cost + (size_t)b * S;
    int n = 0;
    double sum = 0, lo = INFINITY, hi = -INFINITY;
    for (int s = 0; s < S; s++) {
        const double v = cb[s];
        if (isfinite(v)) { n++; sum += v; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    }
    const double mean = sum / n;
    double ss = 0;
    for (int s = 0; s < S; s++) {
        const double v = cb[s];
        if (isfinite(v)) ss += (v - mean) * (v - mean);
    }
    double* o = stats + (size_t)b * ILQR_CL_STATS;
    o[0] = n ? mean : NAN;
    o[1] = n > 1 ? ss / (n - 1) : (n ? 0.0 : NAN);
    o[2] = n ? lo : NAN;
    o[3] = n ? hi : NAN;
    o[4] = (double)(S - n);
}

// ---- ilqr_problem_closed_loop_cov: the covariance of the closed loop, propagated analytically (ilqr_closed_loop_cov.hpp)

// One lane per instance walks the steps.  Sigma, M = F Sigma, G = K Sigma, a row of H = M K' and the time column of B live in an explicit
// per-lane workspace (c.ws, entry e of instance b at ws[e Bp + b], as k_backward's): 225 doubles of Sigma alone would spill.  The lower
// triangle of Sigma' is computed and mirrored, so the workspace -- and every Sigma_k stored from it -- is exactly symmetric.  MAP: a chain of
// fewer than 7 joints; the gain entries of padded rows and columns are read as 0, so the padding takes no part (its Sigma stays 0).
template <class S>
constexpr int cl_cov_ws_doubles() { return 2 * S::NX * S::NX + S::NU * S::NX + S::NU + 2 * S::NX; }
int cl_cov_ws_entries(int kind, int nd) {
    int n = 0;
    SysAll::dispatch(kind, nd, [&](auto s) { n = cl_cov_ws_doubles<decltype(s)>(); });
    return n;
}

template <class S, bool MAP>
__global__ __launch_bounds__(64) void k_cl_cov(Bufs a, ClCovArgs c, IndexMap mx, IndexMap mu) {
    constexpr int NX = S::NX, NU = S::NU, ND = S::ND, TM = S::TM;
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= d.B) return;
    const int Bp = d.Bp, T = d.T, cur = a.cur[b];
    const int nxu = MAP ? mx.n_user : NX, nuu = MAP ? mu.n_user : NU;
    const int sym = a.kd_sym, rowp = kd_rowp(NX), rs = kd_rs(sym, NU, rowp);
    const double* Xb = a.X[cur] + b;  // entry `row` of the plan: Xb[row * Bp]
    const double* Ub = a.U[cur] + b;
    double* const w = c.ws + b;
    constexpr int oS = 0, oM = oS + NX * NX, oG = oM + NX * NX, oH = oG + NU * NX, oC = oH + NU, oV = oC + NX, oEnd = oV + NX;
    static_assert(oEnd == cl_cov_ws_doubles<S>(), "workspace layout");
#define WS(o, i, j, C) w[(size_t)((o) + (i) * (C) + (j)) * Bp]
#define WV(o, i) w[(size_t)((o) + (i)) * Bp]
    auto xu = [&](int i) { return MAP ? mx.usr[i] : i; };   // user index of device state entry i, < 0: padding
    auto uu = [&](int i) { return MAP ? mu.usr[i] : i; };
    auto ctl = [](int r) { return r < DOF ? r : ((ND == 2 && r < 2 * DOF) ? r - DOF : NU - 1); };   // the control of row r (the time row: the time control)
    NOUNR for (int i = 0; i < NX; i++)
        NOUNR for (int j = 0; j < NX; j++) WS(oS, i, j, NX) = (i == j) ? c.sx02[i] : 0.0;
    double zmin = INFINITY, zcon = INFINITY;
    int st = 0;  // step table walk
    for (int k = 0; k < T; k++) {
        // ---- what is read off Sigma_k: the outputs, the margin to the bounds
        if (c.Sigma) {
            double* o = c.Sigma + ((size_t)b * T + k) * nxu * nxu;
            NOUNR for (int i = 0; i < NX; i++)
                NOUNR for (int j = 0; j < NX; j++)
                    if (xu(i) >= 0 && xu(j) >= 0) o[xu(i) * nxu + xu(j)] = WS(oS, i, j, NX);
        }
        if (st < d.steps.n && d.steps.t[st] == k) {
            if (c.kp_Sigma) {
                const int n_kp = d.steps.kp[d.steps.n];
                for (int kpi = d.steps.kp[st]; kpi < d.steps.kp[st + 1]; kpi++) {
                    double* o = c.kp_Sigma + ((size_t)b * n_kp + kpi) * nxu * nxu;
                    NOUNR for (int i = 0; i < NX; i++)
                        NOUNR for (int j = 0; j < NX; j++)
                            if (xu(i) >= 0 && xu(j) >= 0) o[xu(i) * nxu + xu(j)] = WS(oS, i, j, NX);
                }
            }
            st++;
        }
        NOUNR for (int i = 0; i < NX; i++) {
            const double sii = WS(oS, i, i, NX);
            if (!(sii > 0)) continue;
            const double xi = Xb[((size_t)k * NX + i) * Bp], sd = sqrt(sii);
            if (d.limits_set && d.lw[i] != 0) zmin = fmin(zmin, fmin(d.smax[i] - xi, xi - d.smin[i]) / sd);
            if (d.lim2 && d.lw2[i] != 0) zmin = fmin(zmin, fmin(d.smax2[i] - xi, xi - d.smin2[i]) / sd);
        }
        if (k == T - 1) break;
        // ---- the step
        const double* rec = KD_REC(a.KD, Bp, rs, k, b);
        auto K = [&](int i, int j) { return (MAP && (mu.usr[i] < 0 || mx.usr[j] < 0)) ? 0.0 : rec[kd_off(sym, rowp, i, j)]; };
        const double* u = Ub + (size_t)k * NU * Bp;  // u_i = u[i Bp]
        if (c.con_var || c.con_z) {  // uniform: the constraint rows of the step, c' Sigma_k c with c = a_x + K' a_u (ilqr_problem_closed_loop_cov_con)
            NOUNR for (int r = 0; r < a.m; r++) {
                const size_t row = (size_t)(a.per_step ? k : 0) * a.m + r;
                const double* Ar = a.conA + row * (NX + NU);
                double mu = 0;   // A_k[r] [xbar_k; ubar_k], in con_g's order
                NOUNR for (int j = 0; j < NX; j++) {
                    double cj = Ar[j];
                    NOUNR for (int i = 0; i < NU; i++) cj += K(i, j) * Ar[NX + i];
                    WV(oV, j) = cj;
                    mu += Ar[j] * Xb[((size_t)k * NX + j) * Bp];
                }
                NOUNR for (int i = 0; i < NU; i++) mu += Ar[NX + i] * u[(size_t)i * Bp];
                double var = 0;
                NOUNR for (int i = 0; i < NX; i++) {
                    double si = 0;
                    NOUNR for (int j = 0; j < NX; j++) si += WS(oS, i, j, NX) * WV(oV, j);
                    var += WV(oV, i) * si;
                }
                if (c.con_var) c.con_var[((size_t)b * (T - 1) + k) * a.m + r] = var;
                if (var > 0) zcon = fmin(zcon, (a.conb[row] - mu) / sqrt(var));
            }
        }
        const double dts = TM ? u[(size_t)(NU - 1) * Bp] : 0.0;
        const double dt = TM ? dts * dts : d.dt;
        const double b1 = (ND == 1) ? dt : dt * dt / 2;   // B on the position rows; dt on the velocity rows
        NOUNR for (int r = 0; r < NX; r++) {
            const bool is_q = r < DOF, is_v = ND == 2 && r >= DOF && r < 2 * DOF, is_t = TM && r == NX - 1;
            const double ui = is_t ? 0.0 : u[(size_t)ctl(r) * Bp], vi = (ND == 2 && is_q) ? Xb[((size_t)k * NX + DOF + r) * Bp] : 0.0;
            WV(oC, r) = TM ? cov_time_col<ND>(is_q, is_v, is_t, dts, ui, vi) : 0.0;
        }
        // G = K Sigma, u_var = diag(G K')
        NOUNR for (int i = 0; i < NU; i++) {
            NOUNR for (int cc = 0; cc < NX; cc++) {
                double s = 0;
                NOUNR for (int j = 0; j < NX; j++) s += K(i, j) * WS(oS, j, cc, NX);
                WS(oG, i, cc, NX) = s;
            }
            if (c.u_var && uu(i) >= 0) {
                double s = 0;
                NOUNR for (int cc = 0; cc < NX; cc++) s += WS(oG, i, cc, NX) * K(i, cc);
                c.u_var[((size_t)b * (T - 1) + k) * nuu + uu(i)] = s;
            }
        }
        // M = F Sigma
        NOUNR for (int r = 0; r < NX; r++) {
            const bool is_q = r < DOF, is_t = TM && r == NX - 1;
            const double br = is_t ? 0.0 : (is_q ? b1 : dt), cr = WV(oC, r);
            NOUNR for (int cc = 0; cc < NX; cc++) {
                double m = WS(oS, r, cc, NX);
                if (ND == 2 && is_q) m += dt * WS(oS, DOF + r, cc, NX);
                if (!is_t) m += br * WS(oG, ctl(r), cc, NX);
                if (TM) m += cr * WS(oG, NU - 1, cc, NX);
                WS(oM, r, cc, NX) = m;
            }
        }
        // Sigma' = M F' + diag(sigma_w^2): the lower triangle, mirrored
        NOUNR for (int r = 0; r < NX; r++) {
            NOUNR for (int i = 0; i < NU; i++) {
                double s = 0;
                NOUNR for (int j = 0; j < NX; j++) s += WS(oM, r, j, NX) * K(i, j);
                WV(oH, i) = s;
            }
            NOUNR for (int cc = 0; cc <= r; cc++) {
                const bool is_q = cc < DOF, is_t = TM && cc == NX - 1;
                double v = WS(oM, r, cc, NX);
                if (ND == 2 && is_q) v += dt * WS(oM, r, DOF + cc, NX);
                if (!is_t) v += (is_q ? b1 : dt) * WV(oH, ctl(cc));
                if (TM) v += WV(oC, cc) * WV(oH, NU - 1);
                if (cc == r) v += c.sw2[r];
                WS(oS, r, cc, NX) = v;
                WS(oS, cc, r, NX) = v;
            }
        }
    }
#undef WS
#undef WV
    if (c.lim_z) c.lim_z[b] = zmin;
    if (c.con_z) c.con_z[b] = zcon;
}

// kp_var[b][kpi][g]: the trace of group g's 3 x 3 block of Jf Sigma_t Jf' (include/ilqr_hip.h), one lane per (instance, keypoint), from
// kp_Sigma [B][n_kp][n_x][n_x] on the USER's dimensions (dof joints: position j at j, velocity at dof + j, the time at ND dof) and the
// geometric Jacobian at the plan's state of the keypoint's step (the object frame rotates a block and keeps its trace: not applied).
// Serves both propagation kernels.
template <class S>
__global__ __launch_bounds__(64) void k_cl_cov_kp(Bufs a, int dof, const double* __restrict__ kp_Sigma, double* __restrict__ kp_var) {
    constexpr int NX = S::NX, ND = S::ND;
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x;
    const int kpi = blockIdx.y, n_kp = d.steps.kp[d.steps.n];
    if (b >= d.B || kpi >= n_kp) return;
    const int Bp = d.Bp, nxu = ND * dof + S::TM;
    const double* Sg = kp_Sigma + ((size_t)b * n_kp + kpi) * nxu * nxu;
    double var[ILQR_CL_COV_KP] = {0, 0, 0, 0, 0};
    bool joint = S::JOINT;
    if (!S::JOINT && ND == 1) joint = d.kp_joint[kpi] != 0;
    if (joint) {
        double s = 0;
        for (int j = 0; j < dof; j++) s += Sg[j * nxu + j];
        var[ILQR_KP_ERR_POS] = s;
    } else {
        const double* X = a.X[a.cur[b]];
        double q[DOF], p3[3], qt[4], J[6][DOF];
        UNR for (int i = 0; i < DOF; i++) q[i] = AT(X, d.kp_t[kpi] * NX + i, b);
        fk<true>(d.chain, q, p3, qt, J);
        // trace(Jh S Jh') = sum_ij S[i][j] (Jh'Jh)[i][j] for the upper (translation) and the lower (rotation) half Jh of J: one pass over the
        // block of Sigma with an entry at a time in flight (the products J S J' held in registers next to FK spilled)
        UNR for (int blk = 0; blk < ND; blk++) {
            const double* Sb = Sg + (size_t)blk * dof * (nxu + 1);   // the (blk, blk) block of Sigma
            double tp = 0, tq = 0;
            UNR for (int i = 0; i < DOF; i++) {
                UNR for (int j = 0; j < DOF; j++) {
                    const double sij = (i < dof && j < dof) ? Sb[i * nxu + j] : 0.0;
                    tp += sij * (J[0][i] * J[0][j] + J[1][i] * J[1][j] + J[2][i] * J[2][j]);
                    tq += sij * (J[3][i] * J[3][j] + J[4][i] * J[4][j] + J[5][i] * J[5][j]);
                }
            }
            var[blk == 0 ? ILQR_KP_ERR_POS : ILQR_KP_ERR_VEL] = tp;
            var[blk == 0 ? ILQR_KP_ERR_ORN : ILQR_KP_ERR_ANGVEL] = tq;
        }
    }
    if (S::TM) var[ILQR_KP_ERR_TIME] = Sg[(nxu - 1) * nxu + nxu - 1];
    double* o = kp_var + ((size_t)b * n_kp + kpi) * ILQR_CL_COV_KP;
    UNR for (int g = 0; g < ILQR_CL_COV_KP; g++) o[g] = var[g];
}

// f(X) for every (instance, timestep): one lane per pair (tuple<1> of ILQRRecursive::solve)
template <class S>
__global__ __launch_bounds__(64) void k_fx_all(Bufs a, double* __restrict__ out /* natural [B][T][NF] */) {
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = blockIdx.y;
    if (b >= d.B) return;
    const int Bp = d.Bp;
    const double* X = a.X[a.cur[b]];
    double x[S::NX], fxv[S::NF];
    UNR for (int i = 0; i < S::NX; i++) x[i] = AT(X, t * S::NX + i, b);
    fx_of<S, false>(d, x, fxv, nullptr);
    UNR for (int i = 0; i < S::NF; i++) out[((size_t)b * d.T + t) * S::NF + i] = fxv[i];
}

// stand-alone batched FK (KDLRobot::updateKinematics), natural layouts
__global__ __launch_bounds__(64) void k_fk_batch(const DevDesc* dd, int n, const double* __restrict__ q, double* __restrict__ pos, double* __restrict__ quat,
                           double* __restrict__ jac) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double qv[DOF], p[3], qt[4], J[6][DOF];
    UNR for (int j = 0; j < DOF; j++) qv[j] = q[(size_t)i * DOF + j];
    fk<true>(dd->chain, qv, p, qt, J);
    if (pos) { UNR for (int j = 0; j < 3; j++) pos[(size_t)i * 3 + j] = p[j]; }
    if (quat) { UNR for (int j = 0; j < 4; j++) quat[(size_t)i * 4 + j] = qt[j]; }
    if (jac) {
        UNR for (int r = 0; r < 6; r++)
            UNR for (int j = 0; j < DOF; j++) jac[((size_t)i * 6 + r) * DOF + j] = J[r][j];
    }
}

// ------------------------------------------------------------------------------------------------ launchers

// the generic kernels exist for every system: SysAll (ilqr_device.hpp)

void launch_kp_derivs(int kind, int nd, const Bufs& a, int B, hipStream_t st, const FwdArgs& f) {
    if (f.n_kp <= 0) return;
    SysAll::dispatch(kind, nd, [&](auto s) {
        using S = decltype(s);
        if (f.shared) {  // f.n_kp = distinct steps, f.n_kp_all = keypoints
            hipLaunchKernelGGL((k_kp_terms<S>), dim3((B + 63) / 64, f.n_kp_all), dim3(64), 0, st, a);
            hipLaunchKernelGGL((k_kp_sum<S>), dim3((B + 63) / 64, f.n_kp), dim3(64), 0, st, a);
        } else if (f.kp_ext) hipLaunchKernelGGL((k_kp_derivs<S, true>), dim3((B + 63) / 64, f.n_kp), dim3(64), 0, st, a, f.fused);
        else hipLaunchKernelGGL((k_kp_derivs<S, false>), dim3((B + 63) / 64, f.n_kp), dim3(64), 0, st, a, f.fused);
    });
}

void launch_gains_prepare(const Bufs& a, int B, hipStream_t st) { hipLaunchKernelGGL(k_gains_prepare, dim3((B + 63) / 64), dim3(64), 0, st, a); }

void launch_gains_al_weights(int kind, int nd, const Bufs& a, int B, int T, double penalty, hipStream_t st) {
    SysAll::dispatch(kind, nd, [&](auto s) {
        hipLaunchKernelGGL((k_gains_al_weights<decltype(s)>), dim3((B + 255) / 256, T - 1), dim3(256), 0, st, a, penalty);
    });
}

void launch_init(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st, double penalty, const ObsArgs* o) {
    SysAll::dispatch(kind, nd, [&](auto s) {
        using S = decltype(s);
        if (o && al) hipLaunchKernelGGL((k_init_rollout<S, true, ObsArgs>), dim3((B + 63) / 64), dim3(64), 0, st, a, penalty, *o);
        else if (o) hipLaunchKernelGGL((k_init_rollout<S, false, ObsArgs>), dim3((B + 63) / 64), dim3(64), 0, st, a, penalty, *o);
        else if (al) hipLaunchKernelGGL((k_init_rollout<S, true>), dim3((B + 63) / 64), dim3(64), 0, st, a, penalty);
        else hipLaunchKernelGGL((k_init_rollout<S, false>), dim3((B + 63) / 64), dim3(64), 0, st, a, penalty);
    });
}

void launch_backward_generic(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st, const ObsArgs* o) {
    SysAll::dispatch(kind, nd, [&](auto s) {
        using S = decltype(s);
        if (o && al) hipLaunchKernelGGL((k_backward<S, true, ObsArgs>), dim3((B + 63) / 64), dim3(64), 0, st, a, *o);
        else if (o) hipLaunchKernelGGL((k_backward<S, false, ObsArgs>), dim3((B + 63) / 64), dim3(64), 0, st, a, *o);
        else if (al) hipLaunchKernelGGL((k_backward<S, true>), dim3((B + 63) / 64), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((k_backward<S, false>), dim3((B + 63) / 64), dim3(64), 0, st, a);
    });
}

void launch_forward_generic(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st, const FwdArgs& f, const ObsArgs* o) {
    SysAll::dispatch(kind, nd, [&](auto s) {
        using S = decltype(s);
        if (o && al)
            hipLaunchKernelGGL((k_forward<S, true, ObsArgs>), dim3((B + 63) / 64), dim3(64), 0, st, a, f.it, f.line_search, f.early_stop, f.penalty_roll,
                               f.penalty_update, f.do_update, f.nb_iter, *o);
        else if (o)
            hipLaunchKernelGGL((k_forward<S, false, ObsArgs>), dim3((B + 63) / 64), dim3(64), 0, st, a, f.it, f.line_search, f.early_stop, f.penalty_roll,
                               f.penalty_update, f.do_update, f.nb_iter, *o);
        else if (al)
            hipLaunchKernelGGL((k_forward<S, true>), dim3((B + 63) / 64), dim3(64), 0, st, a, f.it, f.line_search, f.early_stop, f.penalty_roll,
                               f.penalty_update, f.do_update, f.nb_iter);
        else
            hipLaunchKernelGGL((k_forward<S, false>), dim3((B + 63) / 64), dim3(64), 0, st, a, f.it, f.line_search, f.early_stop, f.penalty_roll,
                               f.penalty_update, f.do_update, f.nb_iter);
    });
}

void launch_obs_derivs(const Bufs& a, const ObsArgs& o, int B, int T, int nx, int all, hipStream_t st) {
    for (int k0 = 0; k0 < T; k0 += 65535) {   // the y extent of a grid
        const int rows = T - k0 < 65535 ? T - k0 : 65535;
        hipLaunchKernelGGL(k_obs_derivs, dim3((B + 63) / 64, rows), dim3(64), 0, st, a, o, nx, k0, all);
    }
}
void launch_obs_query(const ObsArgs& o, int B, int Bp, int T, int dof, double* cost, double* lx, double* lxx, hipStream_t st) {
    hipLaunchKernelGGL(k_obs_query, dim3((B + 255) / 256, T), dim3(256), 0, st, (const double*)o.obd, B, Bp, T, dof, cost, lx, lxx);
}

void launch_fx_all(int kind, int nd, const Bufs& a, int B, int T, double* out, hipStream_t st) {
    const dim3 grid((B + 63) / 64, T), block(64);
    SysAll::dispatch(kind, nd, [&](auto s) { hipLaunchKernelGGL((k_fx_all<decltype(s)>), grid, block, 0, st, a, out); });
}

void launch_to_soa(const double* src, double* dst, int B, int Bp, int rows, hipStream_t st) {
    hipLaunchKernelGGL(k_to_soa, dim3((B + 255) / 256, rows), dim3(256), 0, st, src, dst, B, Bp, rows);
}
void launch_from_soa(const double* src, double* dst, int B, int Bp, int rows, hipStream_t st) {
    hipLaunchKernelGGL(k_from_soa, dim3((B + 255) / 256, rows), dim3(256), 0, st, src, dst, B, Bp, rows);
}
void launch_from_soa_cur(const double* s0, const double* s1, const int* cur, double* dst, int B, int Bp, int rows, hipStream_t st) {
    hipLaunchKernelGGL(k_from_soa_cur, dim3((B + 255) / 256, rows), dim3(256), 0, st, s0, s1, cur, dst, B, Bp, rows);
}
void launch_from_soa_scaled(const double* src, const double* alpha, const int* iters, double* dst, int B, int Bp, int rows, hipStream_t st) {
    hipLaunchKernelGGL(k_from_soa_scaled, dim3((B + 255) / 256, rows), dim3(256), 0, st, src, alpha, iters, dst, B, Bp, rows);
}
void launch_get_gains(const double* kd, int kd_sym, const double* alpha, const int* iters, double* K_out, double* d_out, int B, int Bp, int T1, int nu, int nx,
                       hipStream_t st) {
    hipLaunchKernelGGL(k_get_gains, dim3((B + 63) / 64, T1), dim3(64), 0, st, kd, kd_sym, alpha, iters, K_out, d_out, B, Bp, T1, nu, nx);
}
void launch_warm_start(const Bufs& a, double* U0, double* q0, double* dq0, int shift, int B, int T, int nx, int nu, int nd, hipStream_t st) {
    hipLaunchKernelGGL(k_warm_start, dim3((B + 63) / 64, T - 1), dim3(64), 0, st, a, U0, q0, dq0, shift, nx, nu, nd);
}
void launch_track(const Bufs& a, const double* x_meas, int k, int with_ff, double* u_out, int B, int nx, int nu, hipStream_t st) {
    hipLaunchKernelGGL(k_track, dim3((B + 63) / 64), dim3(64), 0, st, a, x_meas, k, with_ff, u_out, nx, nu);
}
void launch_closed_loop(int kind, int nd, const Bufs& a, const ClArgs& c, int B, const DofMap* m, hipStream_t st) {
    const dim3 grid(((unsigned)B * c.S + 63) / 64), block(64);
    SysAll::dispatch(kind, nd, [&](auto s) {
        using S = decltype(s);
        if (m && c.con_max) hipLaunchKernelGGL((k_closed_loop<S, true, true>), grid, block, 0, st, a, c, m->x, m->u);
        else if (m) hipLaunchKernelGGL((k_closed_loop<S, true, false>), grid, block, 0, st, a, c, m->x, m->u);
        else if (c.con_max) hipLaunchKernelGGL((k_closed_loop<S, false, true>), grid, block, 0, st, a, c, IndexMap{}, IndexMap{});
        else hipLaunchKernelGGL((k_closed_loop<S, false, false>), grid, block, 0, st, a, c, IndexMap{}, IndexMap{});
    });
}
void launch_closed_loop_cov(int kind, int nd, const Bufs& a, const ClCovArgs& c, int B, const DofMap* m, hipStream_t st) {
    const dim3 grid((B + 63) / 64), block(64);
    SysAll::dispatch(kind, nd, [&](auto s) {
        using S = decltype(s);
        if (m) hipLaunchKernelGGL((k_cl_cov<S, true>), grid, block, 0, st, a, c, m->x, m->u);
        else hipLaunchKernelGGL((k_cl_cov<S, false>), grid, block, 0, st, a, c, IndexMap{}, IndexMap{});
    });
}
void launch_closed_loop_cov_kp(int kind, int nd, const Bufs& a, int B, int n_kp, int dof, const double* kp_Sigma, double* kp_var, hipStream_t st) {
    if (n_kp <= 0) return;
    const dim3 grid((B + 63) / 64, n_kp), block(64);
    SysAll::dispatch(kind, nd, [&](auto s) { hipLaunchKernelGGL((k_cl_cov_kp<decltype(s)>), grid, block, 0, st, a, dof, kp_Sigma, kp_var); });
}
void launch_closed_loop_stats(const double* cost, int B, int S, double* stats, hipStream_t st) {
    hipLaunchKernelGGL(k_closed_loop_stats, dim3((B + 63) / 64), dim3(64), 0, st, cost, B, S, stats);
}
void launch_closed_loop_kp_err(int kind, int nd, const Bufs& a, int B, int S, int n_kp, const double* kpx, double* kp_err, hipStream_t st) {
    if (n_kp <= 0) return;
    const dim3 grid((unsigned)(((size_t)B * S + 63) / 64), n_kp), block(64);
    SysAll::dispatch(kind, nd, [&](auto s) { hipLaunchKernelGGL((k_closed_loop_kp_err<decltype(s)>), grid, block, 0, st, a, S, kpx, kp_err); });
}
void launch_closed_loop_kp_stats(const double* kp_err, const ilqr_cl_tol& tol, int B, int S, int n_kp, double* kp_stats, hipStream_t st) {
    if (n_kp <= 0) return;
    hipLaunchKernelGGL(k_closed_loop_kp_stats, dim3((B + 63) / 64, n_kp), dim3(64), 0, st, kp_err, tol, B, S, n_kp, kp_stats);
}
void launch_closed_loop_con_stats(const double* con_max, const double* con_steps, double con_tol, int B, int S, double* con_stats, hipStream_t st) {
    hipLaunchKernelGGL(k_closed_loop_con_stats, dim3((B + 63) / 64), dim3(64), 0, st, con_max, con_steps, con_tol, B, S, con_stats);
}
void launch_closed_loop_outcome_con(const double* cost, const double* kp_err, const double* lim_cost, const double* con_max, const ilqr_cl_tol& tol,
                                    double con_tol, int B, int S, int n_kp, double* outcome_con, hipStream_t st) {
    hipLaunchKernelGGL(k_closed_loop_outcome_con, dim3((B + 63) / 64), dim3(64), 0, st, cost, kp_err, lim_cost, con_max, tol, con_tol, B, S, n_kp,
                       outcome_con);
}
void launch_closed_loop_outcome(const double* cost, const double* kp_err, const double* lim_cost, const ilqr_cl_tol& tol, int B, int S, int n_kp,
                                double* outcome, hipStream_t st) {
    hipLaunchKernelGGL(k_closed_loop_outcome, dim3((B + 63) / 64), dim3(64), 0, st, cost, kp_err, lim_cost, tol, B, S, n_kp, outcome);
}
void launch_fk_batch(const DevDesc* dd, int n, const double* q, double* pos, double* quat, double* jac, hipStream_t st) {
    hipLaunchKernelGGL(k_fk_batch, dim3((n + 63) / 64), dim3(64), 0, st, dd, n, q, pos, quat, jac);
}

void launch_to_soa_map(const double* src, double* dst, int B, int Bp, int outer, const IndexMap& m, hipStream_t st) {
    hipLaunchKernelGGL(k_to_soa_map, dim3((B + 255) / 256, outer * m.n_dev), dim3(256), 0, st, src, dst, B, Bp, m);
}
void launch_from_soa_cur_map(const double* s0, const double* s1, const int* cur, double* dst, int B, int Bp, int outer, const IndexMap& m, hipStream_t st) {
    hipLaunchKernelGGL(k_from_soa_cur_map, dim3((B + 255) / 256, outer * m.n_user), dim3(256), 0, st, s0, s1, cur, dst, B, Bp, m);
}
void launch_get_gains_map(const double* kd, int kd_sym, const double* alpha, const int* iters, double* K_out, double* d_out, int B, int Bp, int T1,
                          const DofMap& m, hipStream_t st) {
    hipLaunchKernelGGL(k_get_gains_map, dim3((B + 63) / 64, T1), dim3(64), 0, st, kd, kd_sym, alpha, iters, K_out, d_out, B, Bp, T1, m.x, m.u);
}
void launch_track_map(const Bufs& a, const double* x_meas, int k, int with_ff, double* u_out, int B, const DofMap& m, hipStream_t st) {
    hipLaunchKernelGGL(k_track_map, dim3((B + 63) / 64), dim3(64), 0, st, a, x_meas, k, with_ff, u_out, m.x, m.u);
}

}  // namespace ilqr
