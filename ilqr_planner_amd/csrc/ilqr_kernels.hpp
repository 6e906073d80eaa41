// ilqr_kernels.hpp -- device buffer table + kernel launchers shared by ilqr_kernels.hip and the units of the C ABI (ilqr_capi_*.cpp)
#pragma once
#include <hip/hip_runtime.h>

#include "ilqr_device.hpp"
#include "ilqr_dofmap.hpp"

namespace ilqr {

struct ObsArgs;     // ilqr_obstacle.hpp: a problem's obstacle terms; a null pointer below = the problem has none
struct ObsProblem;  // ilqr_obstacle.hpp: ObsArgs with what the host alone reads

// All trajectory-like buffers are [row][Bp] with the (padded) batch innermost; row = t * DIM + component.
struct Bufs {
    const DevDesc* desc;
    double* X[2];  // [T][NX][Bp]   double-buffered; cur[b] says which one holds instance b's accepted trajectory
    double* U[2];  // [T-1][NU][Bp]
    const double* U0;  // [T-1][NU][Bp]
    double* KD;    // gains, one record per (timestep, instance): [T-1][Bp][NU][ROWP], row i = { K_k[i][0..NX-1], d_k[i], pad };
                   // ROWP = NX+1 rounded up to even, so rows are 16-byte aligned: the cooperative kernels read a gain row
                   // with 16-byte loads and the sweep writes an instance's block as one contiguous 448-byte run
    const double* q0;   // [DOF][Bp]
    const double* dq0;  // [DOF][Bp]
    const double* kp_tg;  // [n_kp][NF][Bp]
    double* cost;   // [Bp]
    double* alpha;  // [Bp]
    int* cur;
    int* active;
    int* iters;
    int* status;
    double* kpd;    // [n_kp][NX + NX*NX][Bp] l_x | l_xx of the keypoint steps of the current trajectory (k_kp_derivs)
    int* pend;      // [Bp] line-search winner index + 1 still to be applied by the APPLY pass (0 = nothing pending)
    int* pred;      // [Bp] predicted winner index of the next line search (= winner of the previous iteration)
    double* lsc;    // [16][Bp] limit cost of the alpha = 1 rollout blended to every step size (k_forward_wg -> k_select)
    double* dun;    // [Bp] sum_k ||du_k(1)|| of that rollout
    double* kpdev;  // [n_kp][NX+NU][Bp] deviation (dx, du) of that rollout at the keypoint steps
    double* kpx;    // [n_kp][16][NX+NU][Bp] state | control of every alpha's rollout at the keypoint steps (k_forward_mfma -> k_select_x)
    double* dunA;   // [16][Bp] sum_k ||du_k|| of every alpha's rollout
    double* ws;     // [backward_ws_entries][Bp] matrices of a step of the generic sweep (k_backward), allocated at its first use
    double* cost_trace;   // [nb_iter][Bp] or null
    double* alpha_trace;  // [nb_iter][Bp] or null
    // augmented Lagrangian (shared constraint rows, per-instance multipliers)
    int m, per_step;
    const double* conA;  // [T-1 or 1][m][NX+NU]
    const double* conb;  // [T-1 or 1][m]
    double* lambda;      // [T-1][m][Bp]
    double* Is;          // [T-1][m][Bp]  penalty * active-set mask at rollout time
    int kd_sym;          // the records of KD are in the packed symmetric form of the last solve (see KD_SYM_RS), set by the host per solve
};

constexpr int kd_rowp(int nx) { return (nx + 2) & ~1; }
// Packed record of the single-integrator sweep with uniform control weights (k_backward_si_dpp<.., UNIF = true>): there K = N / dt = ((R + reg) M - I) / dt
// is symmetric (M = S^-1 is, and R + reg is a multiple of I), so the record holds the upper triangle of K row by row (28 entries), d (7) and one pad:
// 36 doubles = 288 bytes instead of 56 = 448.  Gains are 2/3 of what the forward pass reads and 57 % of what the sweep writes.  Entry (i, j), i > j, is
// read as (j, i): the two differ in the last bits (the rows of the swept matrix are formed by different lanes), which the parity gates see as rounding.
constexpr int KD_SYM_RS = 36, KD_SYM_D = 28;
__host__ __device__ constexpr int kd_sym_tri(int i, int j) { return i * 7 - i * (i - 1) / 2 + (j - i); }          // i <= j < 7
__host__ __device__ constexpr int kd_sym_off(int i, int j) { return j >= 7 ? KD_SYM_D + i : (i <= j ? kd_sym_tri(i, j) : kd_sym_tri(j, i)); }  // j = 7: d_i
// offset of entry (i, j) (j = n_x: the feed-forward) in a record of either form, and the record length
__host__ __device__ inline int kd_off(int sym, int rowp, int i, int j) { return sym ? kd_sym_off(i, j) : i * rowp + j; }
__host__ __device__ inline int kd_rs(int sym, int nu, int rowp) { return sym ? KD_SYM_RS : nu * rowp; }
#define KD_REC(kd, Bp, RS, k, b) ((kd) + ((size_t)(k) * (size_t)(Bp) + (size_t)(b)) * (size_t)(RS))

struct FwdArgs {
    int it, line_search, early_stop, do_update, nb_iter;
    int n_kp;     // number of distinct keypoint steps (grid of k_kp_derivs); with unique timesteps the number of keypoints
    int shared;   // some timestep holds more than one keypoint: k_kp_terms + k_kp_sum sum them (generic kernels only, plan_riccati)
    int n_kp_all; // number of keypoints (grid of k_kp_terms)
    int al;       // 1 = AL_ILQR semantics (early stop without the cost test)
    int n_alpha;  // number of step sizes 1, 1/2, ... the line search may try (11 for alpha_floor = 1e-3)
    double penalty_roll, penalty_update;
    int kp_ext;   // some keypoint has a dead zone, an object frame or its own control penalty (selects the full keypoint code)
    int limits;   // the descriptor's limits_set (host copy: selects kernel instantiations)
    int fused;    // the acceptance of the line search is applied by the next sweep (k_backward_si_dpp<.., true>): until then the accepted
                  // trajectory of an instance with pend > 0 is xbar + alpha (x(1) - xbar) over its two buffers
    int fwd_lds;  // Forward::WaveWg runs its predecessor k_forward_wg (the pin ILQR_XC_FWD_WG_LDS) instead of k_forward_reg: same bits
    int fwd_io;   // Forward::WaveWg runs k_forward_reg with its helper waves (RiccatiPlan::fwd_io): same bits
    // RiccatiPlan::obs_dense (null otherwise).  Read by launch_forward_wave alone, on the host, never by a kernel: between the rollout and k_select it
    // runs launch_obs_ls, which adds the obstacle cost of every step size to Bufs::lsc.  obs: the problem's terms; obs_part: [T][16][Bp] scratch;
    // obs_T: the horizon (the descriptor is device memory).
    const ObsProblem* obs;
    double* obs_part;
    int obs_T;
};

// Fused acceptance in the cooperative sweep: what k_apply would have used at the end of the PREVIOUS iteration
struct SweepArgs {
    double pen_in;           // penalty the active-set weights of the incoming trajectory are formed with (AL-ILQR.cpp:190)
    double pen_update_prev;  // penalty of the previous iteration's multiplier update (AL-ILQR.cpp:203-205)
    int do_update_prev;      // the previous iteration was an update iteration
    int si_wg;               // k_backward_si_dpp in its workgroup form (RiccatiPlan::si_wg of the launched half): same bits
    int si_io;               // ... with the I/O wave (RiccatiPlan::si_io of the launched half): same bits
    int si_prep;             // ... and the two preparing waves (RiccatiPlan::si_prep of the launched half): same bits
    const double* sd;        // RiccatiPlan::obs_dense: l_x | l_xx of EVERY step, [T][N + N N][Bp] (k_stage_dense) -> k_backward_si_dpp<.., SW_DENSE>; null otherwise
};

// Launchers of one Riccati iteration; which of them run is decided by plan_riccati (ilqr_plan.hpp).
// generic lane-per-instance kernels (ilqr_kernels.hip)
void launch_init(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st, double penalty, const ObsArgs* o = nullptr);  // k_init_rollout (o: its OBS form)
void launch_gains_prepare(const Bufs& a, int B, hipStream_t st);  // k_gains_prepare: every instance active, alpha = 1 (ilqr_problem_gains)
void launch_gains_al_weights(int kind, int nd, const Bufs& a, int B, int T, double penalty, hipStream_t st);  // k_gains_al_weights: Is of the held plan (ilqr_problem_gains_al, the sweeps that read Is)
void launch_kp_derivs(int kind, int nd, const Bufs& a, int B, hipStream_t st, const FwdArgs& f);  // l_x, l_xx at the keypoint steps (FK + Jacobian), feeding every sweep
void launch_backward_generic(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st, const ObsArgs* o = nullptr);  // k_backward (o: its OBS form, needs launch_obs_derivs first), needs Bufs::ws
int backward_ws_entries(int kind, int nd);  // doubles per instance of k_backward's workspace
void launch_forward_generic(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st, const FwdArgs& f, const ObsArgs* o = nullptr);  // k_forward (o: its OBS form)
// cooperative kernels
void launch_init_lti(int kind, int nd, const Bufs& a, int B, hipStream_t st);  // followed by launch_al_update (it = -1) for AL solves
void launch_backward_si_dpp(bool al, bool fused, bool uniform_R, int lpi, const Bufs& a, int B, hipStream_t st, const SweepArgs& sw);  // rows in registers, DPP broadcasts (ilqr_kernels_dpp.hip)
void launch_backward_rows(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st);  // row-per-lane register sweep (ilqr_kernels_rowsweep.hip); needs launch_kp_derivs first
void launch_backward_mfma(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st);  // needs launch_kp_derivs first
void launch_forward_wave(int kind, bool small, const Bufs& a, int B, hipStream_t st, const FwdArgs& f);  // k_forward_dpp (small) or k_forward_reg (k_forward_wg if f.fwd_lds), + k_select
void launch_apply_wave(int kind, const Bufs& a, int B, int T, hipStream_t st, const FwdArgs& f);  // blend + AL bookkeeping + flip
void launch_forward_lin(const Bufs& a, int B, hipStream_t st, const FwdArgs& f);  // PosOrn-2: k_forward_lin (cost pass of every step size)
void launch_apply_lin(const Bufs& a, int B, int T, hipStream_t st);  // PosOrn-2: the winner re-rolled (k_blend) + flip
void launch_forward_tm(int kind, int nd, const Bufs& a, int B, hipStream_t st, const FwdArgs& f);  // time systems: k_forward_mfma (all step sizes of an instance as one matrix-core product per step) + k_select_x (ilqr_kernels_fwdm.hip)
void launch_apply_tm(int kind, int nd, bool dpp, const Bufs& a, int B, hipStream_t st, const FwdArgs& f);  // time systems: re-roll of the winner, k_apply_dpp_tm (dpp) or k_apply_rows_tm
void launch_al_update(int kind, int nd, const Bufs& a, int B, int T, hipStream_t st, const FwdArgs& f);  // k_al_post: active-set weights (+ multiplier update)
void launch_fx_all(int kind, int nd, const Bufs& a, int B, int T, double* out, hipStream_t st);
void launch_to_soa(const double* src, double* dst, int B, int Bp, int rows, hipStream_t st);
void launch_from_soa(const double* src, double* dst, int B, int Bp, int rows, hipStream_t st);
void launch_from_soa_cur(const double* s0, const double* s1, const int* cur, double* dst, int B, int Bp, int rows, hipStream_t st);
void launch_from_soa_scaled(const double* src, const double* alpha, const int* iters, double* dst, int B, int Bp, int rows, hipStream_t st);
void launch_get_gains(const double* kd, int kd_sym, const double* alpha, const int* iters, double* K_out, double* d_out, int B, int Bp, int T1, int nu, int nx, hipStream_t st);
void launch_warm_start(const Bufs& a, double* U0, double* q0, double* dq0, int shift, int B, int T, int nx, int nu, int nd, hipStream_t st);
void launch_track(const Bufs& a, const double* x_meas, int k, int with_ff, double* u_out, int B, int nx, int nu, hipStream_t st);
void launch_closed_loop_stats(const double* cost, int B, int S, double* stats, hipStream_t st);  // k_closed_loop_stats: stats[B][ILQR_CL_STATS] of cost[B][S]
void launch_fk_batch(const DevDesc* dd, int n, const double* q, double* pos, double* quat, double* jac, hipStream_t st);
// The layout conversions of a chain of fewer than 7 joints (ilqr_dofmap.hpp): the same passes with every per-step vector of `outer`
// vectors widened (upload, padding written as 0) or narrowed (download) through its map.  Rows of the natural side: outer * m.n_user.
void launch_to_soa_map(const double* src, double* dst, int B, int Bp, int outer, const IndexMap& m, hipStream_t st);
void launch_from_soa_cur_map(const double* s0, const double* s1, const int* cur, double* dst, int B, int Bp, int outer, const IndexMap& m,
                             hipStream_t st);  // cur == nullptr: s0
void launch_get_gains_map(const double* kd, int kd_sym, const double* alpha, const int* iters, double* K_out, double* d_out, int B, int Bp, int T1,
                          const DofMap& m, hipStream_t st);
void launch_track_map(const Bufs& a, const double* x_meas, int k, int with_ff, double* u_out, int B, const DofMap& m, hipStream_t st);

}  // namespace ilqr
