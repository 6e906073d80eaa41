// ilqr_closed_loop.hpp -- one lane's pieces of the batched closed-loop rollout (ilqr_problem_closed_loop), shared by the generic kernel
// (k_closed_loop, ilqr_kernels.hip) and the cooperative one (k_closed_loop_coop + k_closed_loop_kp, ilqr_closed_loop.hip): both evaluate the same
// expressions in the same order, so their results are expected to agree bit for bit.
//
//   u_k     = ubar_k + K_k (x_k - xbar_k) [+ alpha d_k]          the tracking law of k_track
//   x_{k+1} = f(x_k, u_k) + w_k                                  dyn_step
//   J       = sum_k limit terms(x_k)  +  sum over the step table of the keypoint terms(x_t, u_t)   (System::cost without AL terms)
#pragma once
#include "../../include/ilqr_hip.h"  // ILQR_MAX_NX, ILQR_CL_STATS
#include "ilqr_closed_loop_plan.hpp"
#include "ilqr_step.hpp"
#include "ilqr_noise.hpp"

namespace ilqr {

// Arguments of a closed-loop launch.  Natural layouts on the user's dimensions; g = b * S + s numbers the (instance, sample) pairs.
struct ClArgs {
    int S;              // samples per instance
    int with_ff;        // add alpha d_k
    const double* x0;   // [B][S][n_x] or null: xbar_0
    const double* w;    // [B][S][T-1][n_x] or null: no disturbance
    double* cost;       // [B][S]
    double* X;          // [B][S][T][n_x] or null
    double* U;          // [B][S][T-1][n_u] or null
    // ilqr_problem_closed_loop_noise: the disturbances and the start perturbation are drawn in the kernel (ilqr_noise.hpp)
    int noise = 0;                          // draw; with 0 the fields below are read by nothing
    unsigned long long seed = 0;
    unsigned int b_off = 0, s_off = 0;      // global index of this call's first instance / sample
    double sigma_w[ILQR_MAX_NX] = {}, sigma_x0[ILQR_MAX_NX] = {};   // user's state layout; 0: no draw for the entry
    double* w_out = nullptr;                // [B][S][T-1][n_x] or null: the disturbance every step added
    // ilqr_problem_closed_loop_report: both null in every other call
    double* kpx = nullptr;                  // generic kernel: the state at every step-table entry, in the cooperative kernel's layout
                                            // [steps.n][n_x + n_u][B * S] (the x rows only); the cooperative kernel has its own argument
    double* lim_cost = nullptr;             // [B][S]: the limit terms of the execution, summed over the steps
    // ilqr_problem_closed_loop_report_con: con_max null in every other call, and the kernels then do not look at the constraint rows
    double con_tol = 0;
    double* con_max = nullptr;              // [B][S]: the maximum of g over the steps and rows, NaN if a g was not finite
    double* con_steps = nullptr;            // [B][S] or null: the steps with a row above con_tol
};

// x_{k+1} += w_k: the caller's w, the draw (nz, on: noise_draw), or both; w_out gets what was added (0 where nothing was).  An entry without
// either is not touched (no + 0.0).  One function for both kernels, like the rest of the step.
template <int NX, bool MAP>
ILQR_DEV void cl_disturb(const ClArgs& c, int g, int k, int T, int nxu, const int* usr, unsigned on, const double* nz, bool valid, double* xn) {
    UNR for (int i = 0; i < NX; i++) {
        const int iu = MAP ? usr[i] : i;
        if (iu < 0) continue;
        double wv = 0.0;
        bool has = false;
        if (c.w) { wv = c.w[(g * (T - 1) + k) * nxu + iu]; has = true; }
        if ((on >> i) & 1u) { wv = has ? wv + nz[i] : nz[i]; has = true; }
        if (has) xn[i] += wv;
        if (c.w_out && valid) c.w_out[(g * (T - 1) + k) * nxu + iu] = has ? wv : 0.0;
    }
}

// The control of one lane at one step.  rec: the step's gain record (entry (i, j) at kd_off, the feed-forward at column n_x); xb, ub: the plan's
// state and control, entry i at xb[i * xs] (xs = Bp in the trajectory buffers, 1 in a staged record); sc: the alpha scaling rule of k_track.
template <class S>
ILQR_DEV void cl_control(const double* rec, int sym, int with_ff, const double* xb, const double* ub, size_t xs, double sc, const double* x, double* u) {
    constexpr int NX = S::NX, NU = S::NU, ROWP = kd_rowp(NX);
    double dx[NX];
    UNR for (int j = 0; j < NX; j++) dx[j] = x[j] - xb[j * xs];
    UNR for (int i = 0; i < NU; i++) {
        double s = ub[i * xs];
        UNR for (int j = 0; j < NX; j++) s += rec[kd_off(sym, ROWP, i, j)] * dx[j];
        if (with_ff) s += sc * rec[kd_off(sym, ROWP, i, NX)];
        u[i] = s;
    }
}

// limit terms of a stage, summed as stage_cost sums them (first set, then the second one)
template <class S>
ILQR_DEV double cl_limits(const DevDesc& d, const double* x) {
    double c = 0;
    if (d.limits_set) c += limit_cost<S>(d, x);
    if (d.lim2) c += lim2_cost<S>(d, x);
    return c;
}

// What an execution carries across its steps for ilqr_problem_closed_loop_report_con: the running maximum of g, the number of steps with a row
// above con_tol, and whether a g was not finite.
struct ClCon {
    double hi = -INFINITY, steps = 0;
    bool bad = false;
};

// The constraint rows of step k at the execution's (x_k, u_k), device layout: g[r] = A_k[r] [x; u] - b_k[r] in con_g's order (state columns
// ascending, control columns ascending, then - b).  A rolled loop over the rows, each row unrolled; the addresses are wave-uniform.  One
// function for both kernels, like the rest of the step.
template <class S>
ILQR_DEV void cl_con(const Bufs& a, double con_tol, int k, const double* x, const double* u, ClCon& cc) {
    double hk = -INFINITY;
    bool bad = false;
    _Pragma("unroll 1") for (int r = 0; r < a.m; r++) {
        const double g = con_g<S>(a, k, r, x, u);
        bad = bad || !isfinite(g);
        hk = (g > hk || g != g) ? g : hk;   // a NaN stays: the step then counts for nothing
    }
    cc.bad = cc.bad || bad;
    cc.hi = hk > cc.hi ? hk : cc.hi;
    if (hk > con_tol) cc.steps += 1.0;
}
// con_max and con_steps of pair g
ILQR_DEV void cl_con_store(const ClArgs& c, int g, const ClCon& cc) {
    c.con_max[g] = cc.bad ? NAN : cc.hi;
    if (c.con_steps) c.con_steps[g] = cc.steps;
}

// acc + the task terms of step-table entry st: every keypoint on the step adds its own, in keypoint order (stage_cost)
template <class S>
ILQR_DEV double cl_kp_terms(const DevDesc& d, const Bufs& a, int b, int st, const double* x, const double* u, double acc) {
    const int Bp = d.Bp;
    for (int kpi = d.steps.kp[st]; kpi < d.steps.kp[st + 1]; kpi++) {
        double tg[S::NF];
        UNR for (int i = 0; i < S::NF; i++) tg[i] = AT(a.kp_tg, kpi * S::NF + i, b);
        acc += kp_cost<S>(d, kpi, tg, x, u);
    }
    return acc;
}

// report: the state of pair g at step-table entry st into c.kpx, the rows the cooperative kernel stores its state in
template <int NX, int NU>
ILQR_DEV void cl_store_kpx(const ClArgs& c, const DevDesc& d, int st, int g, const double* x) {
    const size_t BS = (size_t)d.B * c.S;
    double* o = c.kpx + (size_t)st * (NX + NU) * BS + g;
    UNR for (int i = 0; i < NX; i++) o[(size_t)i * BS] = x[i];
}

// generic kernel (ilqr_kernels.hip); m: the maps of a chain of fewer than 7 joints, or null
void launch_closed_loop(int kind, int nd, const Bufs& a, const ClArgs& c, int B, const DofMap* m, hipStream_t st);
// cooperative kernels (ilqr_closed_loop.hip), 7-joint layouts only; kpx: [steps.n][n_x + n_u][B * S] workspace.  A weak declaration: the host
// builds of the generic kernel set link without that file, and a launch that needs it there is an error (closed_loop, ilqr_capi_closed_loop.cpp).
__attribute__((weak)) void launch_closed_loop_coop(int kind, int nd, const Bufs& a, const ClArgs& c, int B, const ClosedLoopPlan& pl, double* kpx, hipStream_t st);


// ilqr_problem_closed_loop_report (ilqr_kernels.hip), after either rollout.  kpx: the workspace above, filled by the rollout.
// k_closed_loop_kp_err: kp_err[B][S][n_kp][ILQR_KP_ERR] of the states in kpx
void launch_closed_loop_kp_err(int kind, int nd, const Bufs& a, int B, int S, int n_kp, const double* kpx, double* kp_err, hipStream_t st);
// k_closed_loop_kp_stats: kp_stats[B][n_kp][ILQR_KP_STATS] of kp_err (tol travels as a kernel argument)
void launch_closed_loop_kp_stats(const double* kp_err, const ilqr_cl_tol& tol, int B, int S, int n_kp, double* kp_stats, hipStream_t st);
// k_closed_loop_outcome: outcome[B][ILQR_CL_OUTCOME] of cost, kp_err and lim_cost
void launch_closed_loop_outcome(const double* cost, const double* kp_err, const double* lim_cost, const ilqr_cl_tol& tol, int B, int S, int n_kp,
                                double* outcome, hipStream_t st);

// ilqr_problem_closed_loop_report_con (ilqr_kernels.hip), after either rollout
// k_closed_loop_con_stats: con_stats[B][ILQR_CL_CON_STATS] of con_max and con_steps
void launch_closed_loop_con_stats(const double* con_max, const double* con_steps, double con_tol, int B, int S, double* con_stats, hipStream_t st);
// k_closed_loop_outcome_con: outcome_con[B][ILQR_CL_OUTCOME_CON] of cost, kp_err, lim_cost and con_max
void launch_closed_loop_outcome_con(const double* cost, const double* kp_err, const double* lim_cost, const double* con_max, const ilqr_cl_tol& tol,
                                    double con_tol, int B, int S, int n_kp, double* outcome_con, hipStream_t st);

}  // namespace ilqr
