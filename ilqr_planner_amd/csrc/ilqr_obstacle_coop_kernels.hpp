// ilqr_obstacle_coop_kernels.hpp -- the lane-per-item kernels of the obstacle terms' cooperative path (RiccatiPlan::obs_dense) and their launchers,
// declared in ilqr_obstacle.hpp: definitions, included by ilqr_capi_kernels.cpp alone.  That file is compiled as HIP for the product library and as C++
// for the host build of tests/tools/hostsim, so both get them from one text and no list of files changes.  They are NOT in ilqr_kernels.hip beside
// k_obs_derivs: a kernel added there moves every kernel of that unit's code object, and the C3 bench line follows it (ilqr_multistart_kernels.hpp
// has the figures; with these three kernels in that unit the line read 5.5152 ms per step against the parent's 5.4878 in one session).
#pragma once
#include "ilqr_kernels.hpp"
#include "ilqr_obstacle.hpp"
#include "ilqr_step.hpp"

namespace ilqr {

#ifndef UNR
#define UNR _Pragma("unroll")
#endif
#define OC_AT(buf, row, b) (buf)[(size_t)(row) * (size_t)Bp + (size_t)(b)]   // [row][Bp]

// ---- obstacle terms on the cooperative kernels of the single-integrator systems (RiccatiPlan::obs_dense): N = 7 positions are the state

// sd[k] = l_x | l_xx of stage k, one lane per (instance, step), lanes along the batch: every load and store is a whole run of a [row][Bp] row.
// base + obstacle term, in that order: base = the entry of kpd at a keypoint step (one keypoint per step on this path; limits in it), the limit
// terms in k_backward_si_dpp's expressions elsewhere.  Runs behind k_kp_derivs and k_obs_derivs on the accepted trajectory X[cur].
__global__ __launch_bounds__(64) void k_stage_dense(Bufs a, const double* __restrict__ obd, double* __restrict__ sd, int k0, int all) {
    constexpr int N = 7;
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x;
    const int k = k0 + (int)blockIdx.y;   // uniform
    if (b >= d.B) return;
    if (!all && !a.active[b]) return;
    const int Bp = d.Bp;
    int kpi = -1;
    for (int i = 0; i < d.n_kp; i++) kpi = (d.kp_t[i] == k) ? i : kpi;   // uniform
    const double* ob = obd + (size_t)k * OBS_W * (size_t)Bp;
    double* out = sd + (size_t)k * (N + N * N) * (size_t)Bp;
    if (kpi >= 0) {
        const double* src = a.kpd + (size_t)kpi * (N + N * N) * (size_t)Bp;
        UNR for (int i = 0; i < N; i++) OC_AT(out, i, b) = OC_AT(src, i, b) + OC_AT(ob, OBS_LX + i, b);
        UNR for (int i = 0; i < N; i++)
            UNR for (int j = 0; j < N; j++) OC_AT(out, N + i * N + j, b) = OC_AT(src, N + i * N + j, b) + OC_AT(ob, OBS_LXX + (i <= j ? obs_tri(i, j) : obs_tri(j, i)), b);
        return;
    }
    const double* x = a.X[a.cur[b]] + (size_t)k * N * (size_t)Bp;
    const int lim_on = d.limits_set;   // uniform
    UNR for (int i = 0; i < N; i++) {
        double lx = 0.0, lim = 0.0;
        if (lim_on) {   // inspectJointLimit (System.cpp:121-142) as the sweep forms it
            const double xv = OC_AT(x, i, b);
            const double smax_v = d.lw[i] != 0 ? d.smax[i] : __builtin_inf(), smin_v = d.lw[i] != 0 ? d.smin[i] : -__builtin_inf();
            const double beyond = fmax(xv - smax_v, 0.0) + fmax(smin_v - xv, 0.0);
            lim = (beyond > 0.0) ? d.pen_xx : 0.0;
            lx = d.penalty * fmax(xv - smax_v, 0.0) - d.penalty * fmax(smin_v - xv, 0.0);
        }
        OC_AT(out, i, b) = lx + OC_AT(ob, OBS_LX + i, b);
        UNR for (int j = 0; j < N; j++) OC_AT(out, N + i * N + j, b) = (i == j ? lim : 0.0) + OC_AT(ob, OBS_LXX + (i <= j ? obs_tri(i, j) : obs_tri(j, i)), b);
    }
}

// c_obs of step k at step size index i of every active instance, one lane per (instance, step, step size): grid (ceil(B / 64), T, n_alpha), lanes
// along the batch.  The position is k_apply's: x(1) at i = 0, fma(2^-i, x(1) - xbar, xbar) beyond; init: xbar itself (the initial trajectory).
template <bool SELF>
__device__ __forceinline__ void obs_ls_body(const Bufs& a, const ObsArgs& o, double* __restrict__ part, int nx, int k0, int init) {
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x;
    const int k = k0 + (int)blockIdx.y, i = blockIdx.z;   // uniform
    if (b >= d.B) return;
    if (!a.active[b]) return;
    const size_t Bps = (size_t)d.Bp;
    const int cur = a.cur[b];
    const size_t off = (size_t)k * (size_t)nx * Bps + (size_t)b;
    const double* xb = a.X[cur] + off;
    const double* x1 = a.X[1 - cur] + off;
    const double aa = ldexp(1.0, -i);
    const int mode = init ? 0 : (i == 0 ? 1 : 2);   // uniform
    const double c = obs_state<false, SELF>(*o.geom, o.obs + (size_t)(b / o.traj_per_set) * (size_t)o.n_obs * 4, o.n_obs, o.margin, o.weight,
                                      [&](int j) {
                                          if (mode == 0) return xb[(size_t)j * Bps];
                                          const double v1 = x1[(size_t)j * Bps];
                                          if (mode == 1) return v1;
                                          const double vb = xb[(size_t)j * Bps];
                                          return fma(aa, v1 - vb, vb);
                                      },
                                      nullptr, nullptr);
    part[((size_t)k * OBS_LS_ROWS + (size_t)i) * Bps + (size_t)b] = c;
}
__global__ __launch_bounds__(64) void k_obs_ls(Bufs a, ObsArgs o, double* __restrict__ part, int nx, int k0, int init) { obs_ls_body<false>(a, o, part, nx, k0, init); }
__global__ __launch_bounds__(64) void k_obs_ls_self(Bufs a, ObsArgs o, double* __restrict__ part, int nx, int k0, int init) { obs_ls_body<true>(a, o, part, nx, k0, init); }
// k_obs_derivs (ilqr_kernels.hip) for a geometry with self pairs: the same text around obs_state<true, true>.  It lives here and not beside
// k_obs_derivs for the reason at the top of this file: ilqr_kernels.hip's code object is byte for byte what it was before there were self pairs.
__global__ __launch_bounds__(64) void k_obs_derivs_self(Bufs a, ObsArgs o, int nx, int k0, int all) {
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x;
    const int k = k0 + (int)blockIdx.y;
    if (b >= d.B) return;
    if (!all && !a.active[b]) return;
    const size_t Bps = (size_t)d.Bp;
    const double* x = a.X[a.cur[b]] + (size_t)k * (size_t)nx * Bps + (size_t)b;
    double lx[7], lxx[28];
    const double c = obs_state<true, true>(*o.geom, o.obs + (size_t)(b / o.traj_per_set) * (size_t)o.n_obs * 4, o.n_obs, o.margin, o.weight,
                                           [&](int j) { return x[(size_t)j * Bps]; }, lx, lxx);
    double* out = o.obd + (size_t)k * OBS_W * Bps + (size_t)b;
    out[0] = c;
    UNR for (int i = 0; i < 7; i++) out[(size_t)(OBS_LX + i) * Bps] = lx[i];
    UNR for (int e = 0; e < 28; e++) out[(size_t)(OBS_LXX + e) * Bps] = lxx[e];
}
// The sum over the steps in ascending k, one lane per (instance, step size): the order depends on T alone.  Line search: joins the limit cost the
// rollout left in lsc, which select_decide adds to the task cost.  init: joins the initial trajectory's cost behind k_init_finish.
__global__ __launch_bounds__(64) void k_obs_ls_sum(Bufs a, const double* __restrict__ part, int T, int init) {
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y;
    if (b >= d.B) return;
    if (!a.active[b]) return;
    const int Bp = d.Bp;
    double s = 0.0;
    for (int k = 0; k < T; k++) s += OC_AT(part, k * OBS_LS_ROWS + i, b);
    if (init) {
        const double cost = a.cost[b] + s;
        a.cost[b] = cost;
        a.status[b] = isfinite(cost) ? 0 : 1;
    } else {
        OC_AT(a.lsc, i, b) += s;
    }
}

void launch_stage_dense(const Bufs& a, const ObsArgs& o, double* sd, int B, int T, int all, hipStream_t st) {
    for (int k0 = 0; k0 < T; k0 += 65535) {   // the y extent of a grid
        const int rows = T - k0 < 65535 ? T - k0 : 65535;
        hipLaunchKernelGGL(k_stage_dense, dim3((B + 63) / 64, rows), dim3(64), 0, st, a, (const double*)o.obd, sd, k0, all);
    }
}
// ---- the sequential rollouts of the generic set for a geometry with self pairs: the templates of ilqr_rollout_kernels.hpp with ObsSelfArgs.
// obs_state<false, true> is inlined (in ilqr_kernels.hip the pairless term is a call, obs_cost_call): a kernel has the geometry pointer in
// scalar registers, and no function boundary makes it save registers on the stack.  The joint positions are picked by a compare chain on the
// (uniform) joint index: no private array is indexed.
ILQR_DEV double obs_stage_cost(ObsSelfArgs o, int b, const double* x) {
    const double q0 = x[0], q1 = x[1], q2 = x[2], q3 = x[3], q4 = x[4], q5 = x[5], q6 = x[6];
    return obs_state<false, true>(*o.geom, o.obs + (size_t)(b / o.traj_per_set) * (size_t)o.n_obs * 4, o.n_obs, o.margin, o.weight,
                                  [&](int j) { return j == 0 ? q0 : j == 1 ? q1 : j == 2 ? q2 : j == 3 ? q3 : j == 4 ? q4 : j == 5 ? q5 : q6; }, nullptr, nullptr);
}
#include "ilqr_rollout_kernels.hpp"

void launch_init_self(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st, double penalty, const ObsArgs& o) {
    ObsSelfArgs os;
    static_cast<ObsArgs&>(os) = o;
    SysAll::dispatch(kind, nd, [&](auto s) {
        using S = decltype(s);
        if (al) hipLaunchKernelGGL((k_init_rollout<S, true, ObsSelfArgs>), dim3((B + 63) / 64), dim3(64), 0, st, a, penalty, os);
        else hipLaunchKernelGGL((k_init_rollout<S, false, ObsSelfArgs>), dim3((B + 63) / 64), dim3(64), 0, st, a, penalty, os);
    });
}
void launch_forward_generic_self(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st, const FwdArgs& f, const ObsArgs& o) {
    ObsSelfArgs os;
    static_cast<ObsArgs&>(os) = o;
    SysAll::dispatch(kind, nd, [&](auto s) {
        using S = decltype(s);
        if (al)
            hipLaunchKernelGGL((k_forward<S, true, ObsSelfArgs>), dim3((B + 63) / 64), dim3(64), 0, st, a, f.it, f.line_search, f.early_stop, f.penalty_roll,
                               f.penalty_update, f.do_update, f.nb_iter, os);
        else
            hipLaunchKernelGGL((k_forward<S, false, ObsSelfArgs>), dim3((B + 63) / 64), dim3(64), 0, st, a, f.it, f.line_search, f.early_stop, f.penalty_roll,
                               f.penalty_update, f.do_update, f.nb_iter, os);
    });
}
void launch_obs_derivs_self(const Bufs& a, const ObsArgs& o, int B, int T, int nx, int all, hipStream_t st) {
    for (int k0 = 0; k0 < T; k0 += 65535) {   // the y extent of a grid
        const int rows = T - k0 < 65535 ? T - k0 : 65535;
        hipLaunchKernelGGL(k_obs_derivs_self, dim3((B + 63) / 64, rows), dim3(64), 0, st, a, o, nx, k0, all);
    }
}
void launch_obs_ls(const Bufs& a, const ObsProblem& o, double* part, int B, int T, int nx, int n_alpha, int init, hipStream_t st) {
    const int na = init ? 1 : (n_alpha < OBS_LS_ROWS ? n_alpha : OBS_LS_ROWS);
    for (int k0 = 0; k0 < T; k0 += 65535) {   // the y extent of a grid
        const int rows = T - k0 < 65535 ? T - k0 : 65535;
        if (o.n_anchor) hipLaunchKernelGGL(k_obs_ls_self, dim3((B + 63) / 64, rows, na), dim3(64), 0, st, a, o, part, nx, k0, init);
        else hipLaunchKernelGGL(k_obs_ls, dim3((B + 63) / 64, rows, na), dim3(64), 0, st, a, o, part, nx, k0, init);
    }
    hipLaunchKernelGGL(k_obs_ls_sum, dim3((B + 63) / 64, na), dim3(64), 0, st, a, (const double*)part, T, init);
}

#undef OC_AT

}  // namespace ilqr
