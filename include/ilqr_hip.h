/*
 * ilqr_hip.h -- C ABI of the MI355X-native batched iLQR hot path (libilqr_hip.so).
 *
 * The reference (idiap/ilqr_planner) has no FFI layer: its solvers call `sys::System` virtuals in-process
 * and solve ONE problem per call.  This library is what a maintainer binds under the reference's solver
 * classes to solve B independent instances of one System at once on an MI355X.  Each entry point cites the
 * reference interface it replaces (paths relative to ilqr_planner/ilqr_planner in the reference tree).
 *
 * Conventions
 *  - plain C, POD structs, raw pointers + sizes; no C++/torch types.
 *  - every function returning int returns 0 on success, non-zero on error; the message is
 *    ilqr_last_error(ctx).  The C++ host layer turns non-zero into std::runtime_error (the reference's only
 *    error convention, e.g. src/sim/KDLRobot.cpp:49,95; src/system/System.cpp:366).
 *  - host arrays are row-major, batch OUTERMOST ("natural" layout: instance b is what the reference would have
 *    been given / returned for that instance): X[B][T][n_x], U[B][T-1][n_u], K[B][T-1][n_u][n_x] ...
 *    The callee never keeps a host pointer after return.  Device layout is private.
 *  - `*_dev` variants take/return DEVICE pointers in the same natural layout (for callers whose data already
 *    lives in HBM, e.g. torch tensors); all work is enqueued on the context's stream.
 *  - one context per host thread; calls on one context are serialised by the caller.
 *  - all arithmetic is IEEE double, as in the reference (Eigen::MatrixXd everywhere).
 */
#ifndef ILQR_HIP_H
#define ILQR_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ILQR_MAX_SEG 24
#define ILQR_MAX_KP 8
#define ILQR_MAX_NX 15
#define ILQR_MAX_NU 8
#define ILQR_MAX_NF 15
#define ILQR_MAX_NQ 13

/* system kinds: which sys::System subclass is being lowered */
#define ILQR_SYS_POS_ORN 0      /* sys::PosOrnPlannerSys      (src/system/PosOrnPlannerSys.cpp) */
#define ILQR_SYS_POS_ORN_TIME 1 /* sys::PosOrnTimePlannerSys  (src/system/PosOrnTimePlannerSys.cpp) */
#define ILQR_SYS_JOINT 2        /* sys::JointSpacePlannerSys  (src/system/JointSpacePlannerSys.cpp), nb_deriv = 1: target space = joint
                                   space, J = I, AngularKeypoint targets (n_f = n_Q = dof); no chain needed (n_seg may be 0) */
#define ILQR_SYS_JOINT_TIME 3   /* sys::JointSpaceTimePlannerSys (src/system/JointSpaceTimePlannerSys.cpp), nb_deriv = 1: joint space +
                                   time state, dt = u_last^2, AngularTimeKeypoint targets [q*, t*] */

/* per-instance status word */
#define ILQR_STATUS_OK 0
#define ILQR_STATUS_NONFINITE 1   /* accepted cost is NaN/Inf (the reference prints -nan and carries on) */
#define ILQR_STATUS_ALPHA_FLOOR 2 /* last line search bottomed out at alpha <= alpha_floor (accept-anyway rule) */
#define ILQR_STATUS_SWEEP_IO 4    /* a wave of the sweep's I/O-wave form, or of the forward pass's helper-wave form (ILQR_XC_FWD_WG_IO), gave up a bounded wait on its partner (a protocol error, never seen): the instance was \
                                     made inactive, no later kernel of the solve touches it and its outputs are not a solution.  Sticky until the next solve. */

typedef struct ilqr_ctx ilqr_ctx;
typedef struct ilqr_problem ilqr_problem;

/*
 * Flat description of one sys::System + its sim::KDLRobot, shared by all B instances.
 * Replaces what the solvers read through System virtuals:
 *   chain            <- KDLRobot's KDL::Chain after TinyURDFParser + the "robot_custom_tip" segment
 *                       (src/sim/KDLRobot.cpp:45-66): segment s is Trans(xyz) * R * Rot(axis, q[joint]) .
 *   kind,nb_deriv,dt <- System subclass + localInit (src/system/PosOrnPlannerSys.cpp:54-78,
 *                       src/system/PosOrnTimePlannerSys.cpp:50-83)
 *   R_diag           <- System::R (src/system/System.cpp:41,73)
 *   limits_*         <- state_max_/state_min_/joint_limits_weight_/penalty_ (src/system/System.cpp:38-61)
 *   kp_*             <- Keypoint::getTimestep()/getPrecision() (include/ilqr_planner/system/Keypoint.h:23-35);
 *                       timesteps must be non-decreasing.  Keypoint TARGETS are per instance: ilqr_problem_set_keypoint_targets.
 *   reg,alpha_floor,stop_tol <- hard-coded constants of ILQRRecursive.cpp:89,155,174
 */
typedef struct {
    int kind;      /* ILQR_SYS_* */
    int nb_deriv;  /* 1 or 2 */
    int dof;       /* moving joints of the chain: 1..7.  The kernels are built for 7: a chain of fewer joints is solved as the 7-joint
                      problem with inert joints (zero axis, identity transform) behind its last one; every array crossing this ABI keeps
                      the user's layout (n_x, n_u, ... of ilqr_dims_of).  A 6-joint problem costs what a 7-joint one does.  dof < 1,
                      dof > 7 or a chain of another joint count fails with an error text. */
    int horizon;   /* T */
    double dt;     /* PosOrn only; time systems take dt = u_last^2 */
    double R_diag[ILQR_MAX_NU];
    int limits_set;
    double penalty;
    double state_max[ILQR_MAX_NX + 1], state_min[ILQR_MAX_NX + 1];
    int limit_weight[ILQR_MAX_NX + 1];
    int n_seg;
    int seg_joint[ILQR_MAX_SEG];  /* -1 fixed, else joint index */
    double seg_xyz[ILQR_MAX_SEG][3];
    double seg_R[ILQR_MAX_SEG][9]; /* row-major */
    double seg_axis[ILQR_MAX_SEG][3];
    int n_kp;      /* at most ILQR_MAX_KP in all */
    /* Non-decreasing.  Keypoints on the same timestep ADD their terms, each with its own kp_Q, kp_dist, frame, kp_Ru and kp_joint, in index
     * order (a SequentialSystem's sub-systems whose keypoints share a step: SequentialSystem.cpp:115-160 sums them); a shared step needs
     * is_sequence = 1 (or limit_multiplicity > 1), otherwise the timesteps must be strictly ascending.  A plain System keeps only the last
     * keypoint given for a step (System.cpp:78-80,96-101 fill a std::map): its lowering passes that one alone.  Shared steps run on the
     * generic kernels; the batch solvers refuse them with an error text. */
    int kp_timestep[ILQR_MAX_KP];
    double kp_Q[ILQR_MAX_KP][ILQR_MAX_NQ * ILQR_MAX_NQ]; /* row-major n_Q x n_Q, leading dimension n_Q */
    /* PosOrnKeypointDistFunct (src/system/PosOrnKeypointDistFunct.cpp:13-35): dead zones on the residual of keypoint k --
     * position part shrunk by kp_pos_radius towards 0 (0 inside the ball), each orientation component by kp_orn_thresh.
     * kp_dist[k] = 0: plain PosOrnKeypoint (the default; NOT the same as radius 0, which renormalises the residual). */
    int kp_dist[ILQR_MAX_KP];
    double kp_pos_radius[ILQR_MAX_KP];
    double kp_orn_thresh[ILQR_MAX_KP][3];
    /* Object frames and sequential systems.  A keypoint whose sub-system drives the robot through a
     * sim::TransformedSimulationInterface (src/sim/TransformedSimulationInterface.cpp:53-103) sees the pose and the Jacobian in
     * the frame T = [kp_frame_R | kp_frame_p]: p' = R'(p - t), R_ee' = R' R_ee (Eigen quaternion), J' = blkdiag(R,R)' J.
     * kp_has_frame[k] = 0: base frame.  sys::SequentialSystem (src/system/SequentialSystem.cpp:78-168) sums the costs of its
     * sub-systems: every keypoint carries the control penalty of its own sub-system (kp_has_Ru / kp_Ru; the sequential
     * system's own Rt stays in R_diag for l_u, l_uu) and the limit terms are added once per sub-system (limit_multiplicity;
     * 0 = 1).  Sub-systems whose keypoints share a timestep are lowered as keypoints on one step, ordered by sub-system index (each keeps its
     * own residual, frame, dead zone and kp_Ru; the terms add, see kp_timestep).  With limit_multiplicity > 1 the batch solvers
     * (ilqr_solve_batch_cp, ilqr_solve_batch) apply NO limit terms: the reference's SequentialSystem does not override fpBatch, which
     * then runs on the sequence object itself, constructed without limits (SequentialSystem.cpp:12-18). */
    int kp_has_frame[ILQR_MAX_KP];
    double kp_frame_R[ILQR_MAX_KP][9]; /* row-major */
    double kp_frame_p[ILQR_MAX_KP][3];
    int kp_has_Ru[ILQR_MAX_KP];
    double kp_Ru[ILQR_MAX_KP][ILQR_MAX_NU];
    /* Hybrid sequences (HYBRID_SYS*.ipynb): a SequentialSystem may mix a JointSpace(Time)PlannerSys with PosOrn(Time)PlannerSys
     * sub-systems (same state and controls, nb_deriv = 1).  kp_joint[k] = 1 marks keypoint k as the Angular(Time)Keypoint of the
     * joint-space sub-system: target = joint vector (+ continuous time) in the keypoint's n_f slots, residual target - x, J = I
     * (src/system/JointSpacePlannerSys.cpp:77-81), precision n_x x n_x in kp_Q[k] with leading dimension n_x. */
    int kp_joint[ILQR_MAX_KP];
    int limit_multiplicity;
    /* is_sequence: the problem is a sys::SequentialSystem (set by its lowering; limit_multiplicity > 1 implies it): the batch solvers
     * then apply no limit terms.  limits2_set: a second group of sub-systems whose bounds differ from the first group's
     * (HYBRID_SYS_TIME.ipynb gives its two sub-systems (qMax, qMin) and (qMax, -qMax)); every group adds its own limit terms,
     * limit_multiplicity2 times.  Problems with a second group run on the generic one-lane-per-instance kernels. */
    int is_sequence;
    int limits2_set;
    double penalty2;
    double state_max2[ILQR_MAX_NX + 1];
    double state_min2[ILQR_MAX_NX + 1];
    int limit_weight2[ILQR_MAX_NX + 1];
    int limit_multiplicity2;
    /* The three constants below are read by the Riccati solvers (ilqr_solve_recursive, ilqr_solve_al) and by ilqr_problem_gains /
     * ilqr_problem_gains_al, which launch the same sweeps.  The batch solvers (ilqr_solve_batch_cp, ilqr_solve_batch), LQT and the host loop
     * keep the reference's literals whatever is set here.  Away from the defaults: tests/test_gpu_solver_constants.py. */
    double reg;          /* 1e-6.  Added to the diagonal of Quu inside its inverse only, never in the value update (ILQRRecursive.cpp:89); >= 0 */
    double alpha_floor;  /* 1e-3.  The line search halves alpha while alpha > alpha_floor and accepts the first step size at or below it whatever its
                            cost (ILQRRecursive.cpp:155): 1 + ceil(log2(1 / alpha_floor)) step sizes, at most 64.  Up to 16 step sizes
                            (alpha_floor >= 2^-15) are rolled out at once by the cooperative forward passes; below that the plan changes: the
                            generic forward pass tries them one after the other under the same sweeps, and the single-integrator sweep no longer
                            applies the previous winner itself (csrc/ilqr_plan.hpp).  Same results, slower.  > 0 and finite */
    double stop_tol;     /* 1e-3.  Early stop when alpha * sqrt(sum_k |du_k|) < stop_tol (ILQRRecursive.cpp:174, AL-ILQR.cpp:225); the second
                            condition of the non-AL rule, cost < 1e-3, is a literal */
} ilqr_problem_desc;

/* dimensions derived from (kind, nb_deriv, dof): n_x, n_u, n_f (target space), n_Q (residual space) */
typedef struct { int n_x, n_u, n_f, n_Q; } ilqr_dims;
int ilqr_dims_of(const ilqr_problem_desc* desc, ilqr_dims* out);
void ilqr_desc_defaults(ilqr_problem_desc* desc); /* zero + reg/alpha_floor/stop_tol defaults */

/* ---- URDF -> chain (host only, no GPU needed) ------------------------------------------------------------- */
/* What sim::KDLRobot's constructor gets from TinyURDFParser + KDL (src/sim/KDLRobot.cpp:45-66): fills
 * desc->{dof, n_seg, seg_joint, seg_xyz, seg_R, seg_axis} with the joints from base_frame to tip_frame plus the user
 * tool frame Frame(EulerZYX(tool_rpy[0], tool_rpy[1], tool_rpy[2]), tool_xyz) (NULL = identity) as a last fixed
 * segment.  lower/upper (may be NULL) receive the URDF joint limits [dof].  Error text: ilqr_urdf_last_error()
 * ("[KDLRobot] Unable to build kinematic chain from <base> to <tip>" as KDLRobot.cpp:49,56 throws). */
int ilqr_chain_from_urdf(const char* urdf_text, const char* base_frame, const char* tip_frame, const double* tool_rpy,
                         const double* tool_xyz, ilqr_problem_desc* desc, double* lower, double* upper);
const char* ilqr_urdf_last_error(void);

/* ---- context: device + stream + error text -------------------------------------------------------------- */
int ilqr_ctx_create(int device_id, ilqr_ctx** out);
void ilqr_ctx_destroy(ilqr_ctx* ctx);
const char* ilqr_last_error(const ilqr_ctx* ctx);
/* run everything on the caller's hipStream_t (e.g. torch's current stream); NULL = the context's own stream */
int ilqr_ctx_set_stream(ilqr_ctx* ctx, void* hip_stream);
int ilqr_ctx_synchronize(ilqr_ctx* ctx);
/* Large batches of the systems that use the wave-per-instance MFMA sweep are solved as two halves on two internal streams, joined to the
 * context's stream by events (instances are independent: results do not depend on it).  on = 0 keeps every launch on the context's
 * stream, one kernel at a time -- what a profiler run wants.  Default: on (1).  on = 2 splits every cooperative path (experiments only: measured
 * slower on the single-integrator systems).  Any other value fails with an error text.  (No reference counterpart: the reference has no batch.) */
int ilqr_ctx_set_split(ilqr_ctx* ctx, int on);
/* Variant pins of ilqr_ctx_set_crosscheck: AUTO = by batch size; the variants of a pin agree to rounding, not bit for bit, unless said otherwise */
#define ILQR_XC_AUTO 0
#define ILQR_XC_SWEEP_MFMA 1   /* sweep of the 2nd-order / time systems: one instance per wave on the f64 matrix cores (AUTO: up to 2 n_simd instances) */
#define ILQR_XC_SWEEP_ROWS 2   /*   ... 16 lanes per instance with the rows in registers (AUTO: beyond) */
#define ILQR_XC_SWEEP_SI_WAVE 4 /* sweep of the single-integrator systems: k_backward_si_dpp on lone waves at any batch size: the same bits as AUTO (3 is no sweep pin: refused) */
#define ILQR_XC_SWEEP_SI_WG 5   /*   ... in its four-wave workgroup form without the I/O wave (16 lanes per instance only): the same bits as AUTO */
#define ILQR_XC_SWEEP_SI_WG_IO 6 /*  ... in its workgroup form with the I/O wave, a fifth wave that stores the chain waves' gain records and their accepted x, u, the \
                                     latter as whole 128-byte lines (16 lanes per instance, at most one constraint row; ILQR_XC_SWEEP_SI_WG elsewhere; AUTO takes \
                                     it only together with the preparing waves of the next pin): the same bits as AUTO */
#define ILQR_XC_SWEEP_SI_WG_PREP 7 /* ... with the I/O wave and two preparing waves, which load x, u and the multipliers, blend, and form the limit and AL terms \
                                     of every step for the chain waves (where the I/O wave is supported; ILQR_XC_SWEEP_SI_WG_IO's choice elsewhere; AUTO: from \
                                     256 launched instances of an unsplit solve): the same bits as AUTO */
#define ILQR_XC_FWD_WG 1       /* forward pass of the single-integrator systems: the large-batch k_forward_reg (AUTO: beyond 3 n_simd instances) */
#define ILQR_XC_FWD_DPP 2      /*   ... the latency-built k_forward_dpp (AUTO: up to 3 n_simd); agrees with the others to rounding */
#define ILQR_XC_FWD_WG_LDS 3   /*   ... k_forward_wg, the predecessor of k_forward_reg, at any batch size: the same bits as ILQR_XC_FWD_WG (never AUTO) */
#define ILQR_XC_FWD_WG_IO 4    /*   ... k_forward_reg with three helper waves per workgroup that carry its loads and line stores, at any batch size: the same bits as ILQR_XC_FWD_WG, which pins the four-wave form \
                                    (AUTO: where it takes k_forward_reg on an unsplit solve of 1024 to 4096 launched instances) */
#define ILQR_XC_REROLL_ROWS 1  /* re-roll of the line-search winner on the time systems: k_apply_rows_tm (AUTO: beyond n_simd instances) */
#define ILQR_XC_REROLL_DPP 2   /*   ... k_apply_dpp_tm (AUTO: up to n_simd) */
/* Cross-check kernel variants for parity tests (no reference counterpart; the library reads no environment variable -- these are context state,
 * in force for every later solve on the context): generic_kernels = 1 runs ILQRRecursive / AL_ILQR on the generic one-lane-per-instance kernel
 * set instead of the cooperative one; cp_lane_solve = 1 solves the Batch-CP normal equations with one lane per instance instead of one wave;
 * cp_general = 1 sends Batch-CP on the constant-dt systems through the general path of the time systems; sweep, forward and reroll pin one
 * variant each (ILQR_XC_*); a value out of range fails with an error text.  All 0 = the product path.
 * With all three pins at ILQR_XC_AUTO the product path picks between numerically different (rounding-level) kernels by batch size and the
 * device's SIMD count: the same instance can give different bits in batches (or shards) of different sizes.  With all three pinned, the
 * remaining size-dependent choices (the lane grouping and the workgroup form of the single-integrator sweep, the two-stream split) are bit-identical. */
int ilqr_ctx_set_crosscheck(ilqr_ctx* ctx, int generic_kernels, int cp_lane_solve, int cp_general, int sweep, int forward, int reroll);
const char* ilqr_version(void);

/* ---- a batch of B instances of one System ---------------------------------------------------------------- */
int ilqr_problem_create(ilqr_ctx* ctx, const ilqr_problem_desc* desc, int batch, ilqr_problem** out);
void ilqr_problem_destroy(ilqr_problem* p);

/* q0_/dq0_ captured by localInit (PosOrnPlannerSys.cpp:57-58): q0[B][dof], dq0[B][dof] (NULL = zeros) */
int ilqr_problem_set_init_state(ilqr_problem* p, const double* q0, const double* dq0);
/* Keypoint target in f(x) layout [p(3), quat wxyz(4) (, dp(3), dquat(4)) (, t)] : target[B][n_f]
 * (PosOrnKeypoint ctor args, include/ilqr_planner/system/PosOrnKeypoint.h:18-33; SpacetimeKeypoint.h:17-33) */
int ilqr_problem_set_keypoint_targets(ilqr_problem* p, int kp_index, const double* target);
/* U0 of ILQRRecursive::solve / AL_ILQR::solve (include/ilqr_planner/solver/ILQRRecursive.h:36): U0[B][T-1][n_u].
 * Kept on the device so a solve can be repeated from the same start (ilqr_solve_* always restart from it). */
int ilqr_problem_set_controls(ilqr_problem* p, const double* U0);
/* solver::Constraint list + initLambda of AL_ILQR's ctor (include/ilqr_planner/solver/AL-ILQR.h:20-36):
 * A is m x (n_x+n_u), b is m; per_step=0: one (A,b) for every k, else A[T-1][m][n_x+n_u], b[T-1][m];
 * shared by all instances.  lambda0[B][T-1][m] (NULL = zeros). */
int ilqr_problem_set_constraints(ilqr_problem* p, int m, int per_step, const double* A, const double* b, const double* lambda0);
/* put the multipliers back to the lambda0 given to ilqr_problem_set_constraints (= constructing a fresh AL_ILQR) */
int ilqr_problem_reset_multipliers(ilqr_problem* p);
/* device-pointer variants (same layouts, memory already in HBM) */
int ilqr_problem_set_init_state_dev(ilqr_problem* p, const double* q0, const double* dq0);
int ilqr_problem_set_keypoint_targets_dev(ilqr_problem* p, int kp_index, const double* target);
int ilqr_problem_set_controls_dev(ilqr_problem* p, const double* U0);

/* ---- solvers ----------------------------------------------------------------------------------------------- */
/* ILQRRecursive::solve(U0, nb_iter, line_search, early_stop, cb)  (src/solver/ILQRRecursive.cpp:21-181),
 * for all B instances; asynchronous on the context's stream. */
int ilqr_solve_recursive(ilqr_problem* p, int nb_iter, int line_search, int early_stop);
/* AL_ILQR::solve(U0, nb_iter, lag_update_step, penalty, scaling_factor, line_search, early_stop, cb)
 * (src/solver/AL-ILQR.cpp:50-232); multipliers persist in the problem across calls like the reference's
 * `multipliers` member unless re-set with ilqr_problem_set_constraints. */
int ilqr_solve_al(ilqr_problem* p, int nb_iter, int lag_update_step, double penalty, double scaling_factor,
                  int line_search, int early_stop);
/* BatchILQRCP::solve(nb_iter, u0, early_stop, cb) (src/solver/BatchILQRCP.cpp:109-175) with the shared basis
 * PSI ((T-1) n_u x Kw, row-major); u0 = the controls set with ilqr_problem_set_controls.  Kw: any on the constant-dt systems
 * (Kw > 16 through the low-rank form), up to 32 on the time systems.  Keypoints: 1 .. ILQR_MAX_KP at distinct timesteps, for
 * every Kw (the low-rank form solves an m x m system per instance, m = n_kp n_x up to ILQR_MAX_KP n_x). */
int ilqr_solve_batch_cp(ilqr_problem* p, const double* psi, int Kw, int nb_iter, int early_stop);
/* BatchILQR::solve(nb_iter, u0, early_stop, cb) (src/solver/BatchILQR.cpp:110-173): Gauss-Newton on the whole control
 * sequence, i.e. BatchILQRCP with the identity basis (Kw = (T-1) n_u); the identity is never materialised.  Keypoints:
 * 1 .. ILQR_MAX_KP at distinct timesteps on every system (m = n_kp n_x keypoint rows, up to 112 / 120 on the 2nd-order systems). */
int ilqr_solve_batch(ilqr_problem* p, int nb_iter, int early_stop);

/* ---- results (host, natural layout); each synchronises the stream ------------------------------------------ */
int ilqr_problem_get_X(ilqr_problem* p, double* X);       /* [B][T][n_x]     ILQRRecursive tuple<0> */
int ilqr_problem_get_fX(ilqr_problem* p, double* fX);     /* [B][T][n_f]     tuple<1> (one batched FK pass) */
int ilqr_problem_get_U(ilqr_problem* p, double* U);       /* [B][T-1][n_u]   tuple<2> */
int ilqr_problem_get_K(ilqr_problem* p, double* K);       /* [B][T-1][n_u][n_x] tuple<3> */
int ilqr_problem_get_d(ilqr_problem* p, double* d);       /* [B][T-1][n_u]   tuple<4> (scaled by accepted alpha; after ilqr_problem_gains the sweep's d_k itself) */
int ilqr_problem_get_cost(ilqr_problem* p, double* cost); /* [B]             tuple<5> */
int ilqr_problem_get_alpha(ilqr_problem* p, double* alpha); /* [B] last accepted alpha (1.0 after ilqr_problem_gains) */
int ilqr_problem_get_iters(ilqr_problem* p, int* iters);  /* [B] iterations run (early stop) */
int ilqr_problem_get_status(ilqr_problem* p, int* status);/* [B] ILQR_STATUS_* */
int ilqr_problem_get_lambda(ilqr_problem* p, double* lambda); /* [B][T-1][m] */
/* per-iteration stream the reference prints through CallBackMessage ("Iteration i, Cost: c, alpha= a",
 * ILQRRecursive.cpp:167-172): cost_trace/alpha_trace[B][nb_iter] of the last solve (NaN after an early stop) */
int ilqr_problem_get_trace(ilqr_problem* p, double* cost_trace, double* alpha_trace, int nb_iter);
/* device-pointer variants */
int ilqr_problem_get_X_dev(ilqr_problem* p, double* X);
int ilqr_problem_get_U_dev(ilqr_problem* p, double* U);
int ilqr_problem_get_cost_dev(ilqr_problem* p, double* cost);

/* ---- receding horizon and tracking (the uses of the gains the tutorials mention, POS_ORN_SYS.ipynb cell 7; no reference
 * function: ILQRRecursive::solve returns K, k and the caller replays them) -------------------------------------- */
/* The next solve starts from the accepted plan shifted by `shift` timesteps: U0[k] = U[min(k+shift, T-2)] and, for
 * shift > 0, q0 (dq0) = joint part of x_shift -- MPC-style re-planning of the whole batch without leaving HBM. */
int ilqr_problem_warm_start(ilqr_problem* p, int shift);
/* u = ubar_k + K_k (x_meas - xbar_k) [+ alpha d_k if with_feedforward] for every instance:
 * x_meas[B][n_x] -> u_out[B][n_u]; K_k, d_k = the gains ilqr_problem_get_K / get_d return. */
int ilqr_problem_track(ilqr_problem* p, int k, const double* x_meas, int with_feedforward, double* u_out);
int ilqr_problem_track_dev(ilqr_problem* p, int k, const double* x_meas, int with_feedforward, double* u_out);
/* Gains about the plan the problem holds: one backward pass of ILQRRecursive.cpp:68-97 about the X, U that ilqr_problem_get_X / ilqr_problem_get_U
 * return, whichever of the four solvers left them and for any nb_iter, 0 included (ilqr_problem_set_controls, then ilqr_solve_recursive with
 * nb_iter = 0, then this call: gains about an arbitrary control sequence).  The Riccati solvers' own K_k, d_k belong to the plan BEFORE the last
 * step (ILQRRecursive.cpp:68-155 sweeps, then moves the trajectory), and the batch solvers leave none; this call makes K_k, d_k and the plan one.
 *   cost      the system's stage cost: keypoint terms, the limit terms of both limit sets, the descriptor's reg.  No augmented-Lagrangian terms,
 *             also after ilqr_solve_al or with constraints set: it is the sweep ilqr_solve_recursive would run at that trajectory.
 *   writes    K_k, d_k into the problem's gain records, every instance (also those an early stop ended; an instance whose status carries
 *             ILQR_STATUS_NONFINITE or ILQR_STATUS_SWEEP_IO gets unspecified gains, possibly NaN, and keeps its status).  The feed-forward is
 *             unscaled: ilqr_problem_get_d returns the sweep's d_k itself, with_feedforward adds d_k, and ilqr_problem_get_alpha returns 1.0 for
 *             every instance afterwards -- a caller who wants the solver's last step size reads it before this call.
 *   keeps     X, U, fX, cost, iters, status, lambda and the cost / alpha trace, bit for bit.
 *   runs      k_gains_prepare (every instance active, alpha = 1), k_kp_derivs and the sweep chosen for ilqr_solve_recursive(p, 1, 1, 0) on this
 *             problem under the context's pins (batch size, two-stream split and the generic sweep's workspace included); no rollout, no
 *             forward pass.  Under ilqr_profile_enable the call is charged to ILQR_PROF_OTHER and ILQR_PROF_BACKWARD only.
 *   bits      under fixed pins, ilqr_problem_set_controls, a 0-iteration ilqr_solve_recursive and this call give the K of a fresh
 *             ilqr_solve_recursive(p, 1, 1, 0) from the same controls byte for byte, and that solve's d is alpha times this call's, exactly.
 * Afterwards ilqr_problem_track, the closed-loop entry points and their _dev forms accept the problem, until a solver, a setter or
 * ilqr_problem_warm_start changes the plan or its inputs.  Fails unless one of the four solvers has run since the problem's inputs last changed.
 * Asynchronous on the context's stream. */
int ilqr_problem_gains(ilqr_problem* p);
/* The same about the plan of a constrained problem, with the augmented-Lagrangian terms of the rows of ilqr_problem_set_constraints: one backward
 * pass of AL-ILQR.cpp:94-145 about the X, U the problem holds, whichever solver left them (nb_iter = 0 included).  The gains of ilqr_problem_gains
 * pull an execution back to the plan but not to the feasible side; the leftovers of an ilqr_solve_al belong to the trajectory before its last step.
 *   cost      what ilqr_problem_gains sweeps, plus c_u' I c_u, c_u' I c_x, c_x' I c_x on Quu, Qux, Qxx and c' (lambda + I g) on Qu, Qx.
 *   weights   I_k[r] = penalty * ((g_k[r] < 0 && lambda_k[r] == 0) ? 0 : 1) (AL-ILQR.cpp:21-44,190) with g on the held plan and lambda the
 *             multipliers the problem holds now (ilqr_problem_get_lambda).  No multiplier is updated.  `penalty` is the caller's: the one a solve
 *             ended with is penalty0 * scaling^(nb_iter / lag_update_step), formed by repeated multiplication.
 *   writes    K_k, d_k as ilqr_problem_gains does (unscaled feed-forward, ilqr_problem_get_alpha 1.0; instances with ILQR_STATUS_NONFINITE or
 *             ILQR_STATUS_SWEEP_IO get unspecified gains and keep their status), and the internal active-set weights, which every AL solve forms anew.
 *   keeps     X, U, fX, cost, iters, status, lambda and the cost / alpha trace, bit for bit.
 *   runs      k_gains_prepare, k_gains_al_weights where the sweep reads stored weights, k_kp_derivs and the sweep chosen for ilqr_solve_al(p, 1, ..)
 *             on this problem under the context's pins; no rollout, no forward pass, no multiplier update.  ILQR_PROF_OTHER and ILQR_PROF_BACKWARD.
 *   bits      under fixed pins, ilqr_problem_set_constraints(.., lambda), ilqr_problem_set_controls, a 0-iteration ilqr_solve_al and this call give
 *             the K of a fresh ilqr_solve_al(p, 1, 2, penalty, 1.0, 1, 0) from the same inputs byte for byte, and that solve's d is alpha times this call's.
 * Fails without constraint rows, unless a solver has run since the problem's inputs and constraints last changed, and for a penalty that is
 * negative or not finite.  Afterwards as ilqr_problem_gains; a later ilqr_problem_gains overwrites the records with the plain gains. */
int ilqr_problem_gains_al(ilqr_problem* p, double penalty);
/* Closed loop of that law on the plan of the last Riccati solve (or the plan ilqr_problem_gains swept about): n_samples executions of every instance,
 *   x_0 = x0[b][s] (NULL: xbar_0);  u_k = ilqr_problem_track(k, x_k, with_feedforward);  x_{k+1} = f(x_k, u_k) + w[b][s][k] (NULL: none);
 *   cost[b][s] = sum_{k<T-1} cost(x_k, u_k, k) + cost(x_{T-1}, 0, T-1)     (the system's stage cost, no AL terms: what ilqr_solve_recursive reports),
 * with f the system's own step (dt = u_last^2 on the time systems).  Start states and disturbances are the caller's (ilqr_problem_closed_loop_noise draws them on the device).
 * x0[B][S][n_x] or NULL, w[B][S][T-1][n_x] or NULL; cost[B][S]; X[B][S][T][n_x] or NULL; U[B][S][T-1][n_u] or NULL.
 * Fails unless ilqr_solve_recursive / ilqr_solve_al with nb_iter >= 1 or ilqr_problem_gains has run since the problem's inputs last changed (the
 * batch solvers and a 0-iteration solve leave no gains: ilqr_problem_gains computes them about their plan), for n_samples < 1, for a null cost, and when B * n_samples * T * n_x reaches 2^31 (the kernels' 32-bit offsets).
 * _dev: device pointers, asynchronous on the context's stream. */
int ilqr_problem_closed_loop(ilqr_problem* p, int n_samples, const double* x0, const double* w, int with_feedforward, double* cost, double* X,
                             double* U);
int ilqr_problem_closed_loop_dev(ilqr_problem* p, int n_samples, const double* x0, const double* w, int with_feedforward, double* cost, double* X,
                                 double* U);
/* The same rollout with the disturbances and the start-state perturbations drawn inside the kernels, and the costs reduced per instance on
 * the device: no per-step array has to exist, and a call with only `stats` moves the plan in and 5 B doubles out.
 *   x_0 = centre + sigma_x0 .* z,  centre = x0[b][s] (NULL: xbar_0);   x_{k+1} = f(x_k, u_k) + sigma_w .* z_k;   z ~ N(0, 1), independent.
 * The generator is part of this contract, so that a caller can reproduce a draw:
 *   Philox4x32-10: multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85; one round is
 *       p0 = M0 c0, p1 = M1 c2;  c <- (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0));  then k0, k1 += the Weyl constants.
 *   key = (seed & 0xffffffff, seed >> 32);  counter = (instance_offset + b, sample_offset + s, k, j): k = 0 .. T-2 is the step whose
 *       successor is disturbed, k = 0xFFFFFFFF the start-state draw, j the pair index.
 *   One call (r0, r1, r2, r3) gives two normals: u1 = ((double)((r1:r0) >> 11) + 0.5) 2^-53, u2 likewise from r3:r2,
 *       z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2 ln u1) sin(2 pi u2).
 *   Pair j serves entries 2j and 2j + 1 of the state in the user's layout (for an odd n_x the last z1 is dropped; the padded entries of a
 *       chain of fewer than 7 joints get nothing).  Entry i receives sigma[i] z, the product rounded on its own; an entry with sigma 0
 *       receives nothing, and a pair whose sigmas are both 0 is not generated.
 * The draw of (seed, global instance, global sample, step, entry) depends on nothing else: a cut-out of a batch, a shard or a range of samples,
 * run with its offsets, reproduces the large call bit for bit.  Host builds use sin / cos, the device sincospi: they agree to rounding.
 * cost[B][S] or NULL (the per-sample costs then stay in a workspace of the problem); stats[B][ILQR_CL_STATS] or NULL: per instance, over
 * cost[b][0 .. S-1] in sample order, { mean, unbiased variance, min, max } of the finite costs (variance 0 for one, all four NaN for none) and
 * n_bad, the number of costs that are not finite.  X, U as above; w_out[B][S][T-1][n_x] or NULL: the disturbance every step added.
 * Refused: everything ilqr_problem_closed_loop refuses, a null noise, a negative or non-finite sigma, cost and stats both NULL,
 * instance_offset + B or sample_offset + n_samples beyond 2^32.  The 32-bit bound depends on what is asked for: with X, U and w_out all NULL
 * no per-step array exists and the bound is B * n_samples * n_x < 2^31; with any of them it is the one above. */
#define ILQR_CL_STATS 5   /* mean, variance, min, max, n_bad */
typedef struct {
    unsigned long long seed;
    unsigned int instance_offset, sample_offset;   /* this call's first global instance / sample */
    double sigma_w[ILQR_MAX_NX], sigma_x0[ILQR_MAX_NX];   /* user's state layout; 0 = none */
} ilqr_noise;
int ilqr_problem_closed_loop_noise(ilqr_problem* p, int n_samples, const ilqr_noise* noise, const double* x0, int with_feedforward, double* cost,
                                   double* stats, double* X, double* U, double* w_out);
int ilqr_problem_closed_loop_noise_dev(ilqr_problem* p, int n_samples, const ilqr_noise* noise, const double* x0, int with_feedforward, double* cost,
                                       double* stats, double* X, double* U, double* w_out);
/* The same rollout, reporting what every execution did at the keypoints and against the limits -- per sample and reduced per instance on
 * the device; no per-step array has to exist.  The disturbances are the draw above (noise non-NULL), the caller's w[B][S][T-1][n_x] (w
 * non-NULL; both given is refused) or none (both NULL).  A noise whose sigmas are all 0 with n_samples = 1 reports on the plan itself.
 * Keypoint errors.  For keypoint k of the descriptor (0 .. n_kp-1, the descriptor's index, not a step-table entry) on step t_k and the
 *   execution's state x at that step, e is the residual the keypoint's cost term is built from -- f(x) seen through the keypoint's object
 *   frame, then Keypoint::diff (its rule that an all-zero f(x) gives a zero pose residual included) -- WITHOUT the dead zone, which is itself a
 *   tolerance.  Five numbers, ILQR_KP_ERR_*:
 *     POS     ||e[0:3]||_2 (m);  a joint keypoint (the ILQR_SYS_JOINT* kinds, or kp_joint[k]): ||joint-position part of e||_2 (rad) over the user's joints
 *     ORN     ||e[3:6]||_2 (rad: the angle of the reference's log map);  joint keypoint: 0
 *     VEL     ||e[6:9]||_2 for nb_deriv = 2, else 0;  joint keypoint: 0
 *     ANGVEL  ||e[9:12]||_2 for nb_deriv = 2, else 0;  joint keypoint: 0
 *     TIME    |last entry of e| on the time systems, else 0
 * Limit share.  lim_cost[b][s] = the sum over k = 0 .. T-1 of the limit terms of the stage cost at x_k, both limit sets with their
 *   multiplicities: the part of cost[b][s] that is not a keypoint term.  It is 0.0 exactly when no weighted bound was crossed.
 * Tolerances (ilqr_cl_tol).  An execution misses keypoint k if err[k][g] > kp_tol[k][g] for some judged group g; a negative kp_tol[k][g] means
 *   that g is not judged.  It violates the limits if lim_cost > lim_tol (lim_tol >= 0).  Every comparison is strict.
 * Outputs (ilqr_cl_report); each may be NULL, but not all four:
 *   kp_err[B][S][n_kp][ILQR_KP_ERR]     the errors of every sample
 *   kp_stats[B][n_kp][ILQR_KP_STATS]    { mean[5], max[5], n_miss, n_bad } over the samples of instance b in sample order: a sample is bad for
 *                                       keypoint k if one of its five errors is not finite; means and maxima are over the good samples (NaN for
 *                                       none); n_miss counts the good samples that miss keypoint k
 *   lim_cost[B][S]
 *   outcome[B][ILQR_CL_OUTCOME]         { n_ok, n_miss, n_lim, n_bad }: n_bad counts the samples whose cost is not finite (stats[b][4]); among
 *                                       the others n_miss counts those that miss at least one keypoint, n_lim those with lim_cost > lim_tol, n_ok
 *                                       those with neither.  n_ok / n_samples is the plan's success rate.
 * cost[B][S], stats[B][ILQR_CL_STATS]: as above, each may be NULL (the costs then stay in a workspace of the problem); they and the rollout
 * are bit for bit those of the entry points above for the same inputs.  tol may be NULL when neither kp_stats nor outcome is asked for.
 * Refused: everything the entry points above refuse (a null cost is not: see before), noise and w both given, all four report pointers NULL,
 * a NaN tolerance, lim_tol < 0, tol NULL while kp_stats or outcome is asked for.  32-bit bound: no per-step output exists, so without w it is
 * B * n_samples * n_x < 2^31, with w the bound of the caller's w.
 * _dev: every array is a device pointer (noise, tol and out themselves are structs in host memory, read before the call returns);
 * asynchronous on the context's stream. */
#define ILQR_KP_ERR 5
#define ILQR_KP_ERR_POS 0
#define ILQR_KP_ERR_ORN 1
#define ILQR_KP_ERR_VEL 2
#define ILQR_KP_ERR_ANGVEL 3
#define ILQR_KP_ERR_TIME 4
#define ILQR_KP_STATS 12     /* mean[5], max[5], n_miss, n_bad */
#define ILQR_CL_OUTCOME 4    /* n_ok, n_miss, n_lim, n_bad */
typedef struct {
    double kp_tol[ILQR_MAX_KP][ILQR_KP_ERR]; /* execution misses keypoint k if err[k][g] > kp_tol[k][g] for some judged g; negative: g is not judged */
    double lim_tol;                          /* execution violates the limits if lim_cost > lim_tol; >= 0 */
} ilqr_cl_tol;
typedef struct {
    double* kp_err;    /* [B][S][n_kp][ILQR_KP_ERR] or NULL */
    double* kp_stats;  /* [B][n_kp][ILQR_KP_STATS] or NULL */
    double* lim_cost;  /* [B][S] or NULL */
    double* outcome;   /* [B][ILQR_CL_OUTCOME] or NULL */
} ilqr_cl_report;
int ilqr_problem_closed_loop_report(ilqr_problem* p, int n_samples, const ilqr_noise* noise, const double* x0, const double* w,
                                    int with_feedforward, const ilqr_cl_tol* tol, double* cost, double* stats, const ilqr_cl_report* out);
int ilqr_problem_closed_loop_report_dev(ilqr_problem* p, int n_samples, const ilqr_noise* noise, const double* x0, const double* w,
                                        int with_feedforward, const ilqr_cl_tol* tol, double* cost, double* stats, const ilqr_cl_report* out);

/* The Gaussian answer to the same question, without samples: the state covariance of the executions of ilqr_problem_closed_loop_noise
 * (x0 = NULL, no feed-forward term: the covariance about the mean does not depend on it to first order), propagated analytically,
 *   Sigma_0 = diag(sigma_x0^2),   Sigma_{k+1} = F_k Sigma_k F_k' + diag(sigma_w^2),   F_k = A_k + B_k K_k,
 * with K_k the gain ilqr_problem_get_K returns and A_k, B_k the exact Jacobian of the system's step at the plan (xbar_k, ubar_k):
 *   nb_deriv = 1: A = I, B = dt I on the joint rows;   nb_deriv = 2: A = [[I, dt I], [0, I]], B = [[dt^2/2 I], [dt I]];
 *   time systems: dt = s^2 with s = ubar_k's last entry; the time row of A is 1 on the time entry, and the column of B for the last control is
 *   d step / d s: 2 s u_i on the joint rows (nb_deriv = 1), 2 s v_i + 2 s^3 u_i on the position rows with v the velocity BEFORE the step and
 *   2 s u_i on the velocity rows (nb_deriv = 2), 2 s on the time row.  (The reference's solver uses the velocity after the step there; that
 *   is its quirk, not the Jacobian, and is not used here.)
 * On the constant-dt systems the closed loop is linear and the recursion is exact: the sample covariance of ilqr_problem_closed_loop_noise's X
 * converges to Sigma.  On the time systems it is the first-order answer about the plan.
 * sigma_w[n_x], sigma_x0[n_x]: the user's state layout, as in ilqr_noise; NULL: zeros.  Outputs (ilqr_cl_cov), each may be NULL, but not all:
 *   Sigma[B][T][n_x][n_x]        Sigma_0 holds sigma_x0^2 exactly; every Sigma_k is stored exactly symmetric (one triangle, mirrored)
 *   kp_Sigma[B][n_kp][n_x][n_x]  Sigma at the step of keypoint k of the descriptor
 *   kp_var[B][n_kp][ILQR_CL_COV_KP]  the first-order variance of the task-space deviation at keypoint k, by the groups of
 *                                ilqr_problem_closed_loop_report: the trace of group g's 3 x 3 block of Jf Sigma_t Jf', Jf = blkdiag(J, J) bordered
 *                                by 1 for the time state, J the geometric Jacobian at xbar_t (m^2, rad^2, (m/s)^2, (rad/s)^2, s^2; an object
 *                                frame rotates a block and keeps its trace; dead zones play no part).  A joint keypoint (the ILQR_SYS_JOINT*
 *                                kinds, or kp_joint[k]): POS = the trace of the joint-position block of Sigma_t over the user's joints, ORN =
 *                                VEL = ANGVEL = 0.  VEL = ANGVEL = 0 for nb_deriv = 1; TIME = Sigma_t[time][time], 0 off the time systems.
 *   u_var[B][T-1][n_u]           diag(K_k Sigma_k K_k'): the variance of the commanded controls
 *   lim_z[B]                     how many standard deviations the plan keeps from its bounds: the minimum over k = 0 .. T-1 and the state
 *                                entries i with a weighted bound in either limit set and Sigma_k[i][i] > 0 of
 *                                min(smax_i - xbar_k,i, xbar_k,i - smin_i) / sqrt(Sigma_k[i][i]) (the bounds of that set); +inf if there is no
 *                                such (k, i), negative where the plan itself lies outside a bound.
 * Two kernels serve the call (under ilqr_ctx_set_crosscheck's generic_kernels pin and for chains of fewer than 7 joints: one lane per instance;
 * otherwise rows of Sigma in the registers of 16 lanes).  They sum in different orders: their results agree to rounding, not bit for bit; the
 * second keeps a lane's whole row inside the recursion and makes Sigma symmetric where it is stored.  No expected cost: the limit terms
 * are not smooth, and `stats` of ilqr_problem_closed_loop_noise stays the answer for cost.
 * Refused: what ilqr_problem_closed_loop refuses about the state of the problem, a negative or non-finite sigma, out NULL or all five outputs
 * NULL, B T n_x^2 >= 2^31 when Sigma is asked for, B n_kp n_x^2 >= 2^31 when kp_Sigma is.
 * _dev: the arrays inside `out` are device pointers (the sigmas and out itself are read on the host before the call returns); asynchronous on
 * the context's stream. */
#define ILQR_CL_COV_KP ILQR_KP_ERR   /* POS, ORN, VEL, ANGVEL, TIME: the groups of ilqr_problem_closed_loop_report */
typedef struct {
    double* Sigma;     /* [B][T][n_x][n_x] or NULL */
    double* kp_Sigma;  /* [B][n_kp][n_x][n_x] or NULL: Sigma at the step of descriptor keypoint k */
    double* kp_var;    /* [B][n_kp][ILQR_CL_COV_KP] or NULL */
    double* u_var;     /* [B][T-1][n_u] or NULL: diag(K_k Sigma_k K_k') */
    double* lim_z;     /* [B] or NULL */
} ilqr_cl_cov;
int ilqr_problem_closed_loop_cov(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out);
int ilqr_problem_closed_loop_cov_dev(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out);

/* The two answers above, judged against the inequality rows of ilqr_problem_set_constraints: the only hard constraints of the library, which
 * neither cost, kp_err nor lim_cost look at.  Rows are (A_k, b_k) exactly as ilqr_problem_set_constraints received them: m rows on the user's
 * [x; u] layout, the same rows for every k with per_step = 0.  For execution (b, s) and control step k = 0 .. T-2
 *   g[k][r] = sum_j A_k[r][j] x_k[j] + sum_i A_k[r][n_x + i] u_k[i] - b_k[r]
 * with x_k the execution's state and u_k the commanded control (what the U output of the rollout holds): AL_ILQR::constraints
 * (AL-ILQR.cpp:21-44) on the executed trajectory.  g <= 0 is feasible; x_{T-1} has no control and is not judged, as in the reference.  The
 * summation order is fixed -- state columns ascending, then control columns ascending, then - b_k[r] -- and is the same in both rollout kernels.
 *
 * Sampled: ilqr_problem_closed_loop_report_con.  The arguments of ilqr_problem_closed_loop_report, then con_tol and the outputs (ilqr_cl_con);
 * `out` may be NULL here.  One rollout; cost, stats and the four outputs of `out` are bit for bit those of ilqr_problem_closed_loop_report.
 *   con_max[B][S]                    the maximum of g[k][r] over k and r: <= 0 means feasible throughout; NaN if any g of the execution is not finite
 *   con_steps[B][S]                  the number of steps k with max_r g[k][r] > con_tol (strict), stored as a double
 *   con_stats[B][ILQR_CL_CON_STATS]  { mean con_max, max con_max, mean con_steps, max con_steps, n_con, n_bad } over the samples of instance b in
 *                                    sample order: a sample is bad if its con_max is not finite; means and maxima are over the good samples (NaN
 *                                    for none); n_con counts the good samples with con_max > con_tol
 *   outcome_con[B][ILQR_CL_OUTCOME_CON]  { n_ok, n_miss, n_lim, n_con, n_bad }: n_bad, n_miss and n_lim exactly as in `outcome`; n_con counts the
 *                                    finite-cost samples whose con_max exceeds con_tol or is not finite; n_ok those with none of the three.
 *                                    Needs tol.
 * Each may be NULL; not all four unless `out` asks for something.  No per-step output exists: the 32-bit bounds are those of the report call.
 * Refused: everything ilqr_problem_closed_loop_report refuses (a NULL `out` is not), no constraints set, a NaN con_tol, outcome_con without
 * tol, con and out both asking for nothing.
 *
 * Analytic: ilqr_problem_closed_loop_cov_con.  In the closed loop u - ubar = K_k (x - xbar), so to first order row r at step k has variance
 *   con_var[k][r] = c' Sigma_k c,   c = A_k[r][0:n_x]' + K_k' A_k[r][n_x:]'
 * with Sigma_k and K_k those of ilqr_problem_closed_loop_cov (exact on the constant-dt systems, where the loop is linear).
 *   con_var[B][T-1][m]   the variance above
 *   con_z[B]             how many standard deviations the plan keeps from its constraints: the minimum over k <= T-2 and the rows with
 *                        con_var > 0 of (b_k[r] - A_k[r] [xbar_k; ubar_k]) / sqrt(con_var[k][r]); +inf if there is no such (k, r), negative where
 *                        the plan itself violates a row
 * `out` may be NULL; what it asks for is what ilqr_problem_closed_loop_cov returns, bit for bit per kernel.  Refused: what that call refuses
 * (a NULL `out` is not), no constraints set, con and out both asking for nothing.
 * _dev forms: as above. */
#define ILQR_CL_CON_STATS 6     /* mean con_max, max con_max, mean con_steps, max con_steps, n_con, n_bad */
#define ILQR_CL_OUTCOME_CON 5   /* n_ok, n_miss, n_lim, n_con, n_bad */
typedef struct {
    double* con_max;      /* [B][S] or NULL */
    double* con_steps;    /* [B][S] or NULL */
    double* con_stats;    /* [B][ILQR_CL_CON_STATS] or NULL */
    double* outcome_con;  /* [B][ILQR_CL_OUTCOME_CON] or NULL */
} ilqr_cl_con;
int ilqr_problem_closed_loop_report_con(ilqr_problem* p, int n_samples, const ilqr_noise* noise, const double* x0, const double* w,
                                        int with_feedforward, const ilqr_cl_tol* tol, double* cost, double* stats, const ilqr_cl_report* out,
                                        double con_tol, const ilqr_cl_con* con);
int ilqr_problem_closed_loop_report_con_dev(ilqr_problem* p, int n_samples, const ilqr_noise* noise, const double* x0, const double* w,
                                            int with_feedforward, const ilqr_cl_tol* tol, double* cost, double* stats, const ilqr_cl_report* out,
                                            double con_tol, const ilqr_cl_con* con);
typedef struct {
    double* con_var;  /* [B][T-1][m] or NULL */
    double* con_z;    /* [B] or NULL */
} ilqr_cl_cov_con;
int ilqr_problem_closed_loop_cov_con(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out,
                                     const ilqr_cl_cov_con* con);
int ilqr_problem_closed_loop_cov_con_dev(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out,
                                         const ilqr_cl_cov_con* con);

/* Analytic: ilqr_problem_closed_loop_cov_clr.  The same covariance, judged against the surroundings: the first-order variance of every clearance
 * pair of "clearance" (below) and how many standard deviations the plan keeps from `margin`.  ilqr_clr_robot and ilqr_clr_world are declared
 * below with the clearance calls; this paragraph uses their definitions.
 * Pairs and gradient.  Robot, planes, obstacle sets (instance b reads set b / traj_per_set, n = B; stats_group is not read), self pairs,
 *   margin = world->margin, the pair clearances clr_ij(q), clr_ab(q) and the pair numbering j (obstacles, then planes at n_obs + l, then the self
 *   pair (a, b) as (i, j) = (b, n_obs + n_planes + a)) are exactly those of "clearance".  The gradient grad_ij = n_ij' Jp_i(q) is that of "obstacle
 *   terms": n_ij = (p_i - o_j) / |p_i - o_j| for an obstacle, plane_n[l] for a plane, column m of Jp_i = a_m x (p_i - r_m) for the joints m that
 *   move sphere i's link and 0 for the others; for a self pair grad_ab = n_ab' (Jp_b - Jp_a), n_ab = (p_b - p_a) / |p_b - p_a|: entry m is
 *   n_ab . (a_m x (p_b - r_m)) for the joints that move b's link but not a's and exactly 0 for every other joint (a joint that moves both moves them
 *   rigidly; the library writes that 0, it does not compute and cancel).  The gradient is zero where the two centres coincide.  q is the first dof
 *   entries of xbar_k (the plan ilqr_problem_get_X returns) in the user's layout; velocities and the time state get gradient 0.  Every system kind,
 *   nb_deriv 1 and 2, chains of 1 to 7 joints.
 * Per pair, at step k = 0 .. T-1:
 *   var_ij[k] = grad' Sigma_k[q,q] grad, Sigma_k[q,q] the leading dof x dof block of the Sigma_k ilqr_problem_closed_loop_cov returns for the same
 *     sigmas.  Summation order: s = 0; rows i ascending, within a row the columns j ascending, s = s + (grad_i * Sigma_k[i][j]) * grad_j; one
 *     rounding per operation, no contraction.  A sum that rounding leaves below 0 counts as 0.
 *   z_ij[k] = (clr_ij - margin) / sqrt(var_ij) where var_ij > 0; where var_ij == 0, z_ij = +inf if clr_ij >= margin, else -inf.
 * Per step:
 *   clr_z[B][T]    the minimum of z_ij over the step's pairs (every sphere against the active obstacles of the set and the planes, and the self
 *                  pairs); ties go to the lowest i, then the lowest j.  +inf without any pair.
 *   clr_var[B][T]  var_ij of the pair that attains clr_z; 0 without any pair, and 0 where clr_z is +inf (only a pair with var_ij == 0 has it).
 *   A bad step, as "clearance" defines it, gives NaN in both; so does a step with an entry of Sigma_k[q,q] that is not finite.
 * Per plan:
 *   clr_z_min[B], clr_z_at[B][3] = (k, i, j) (ints): the minimum over the steps in the total order "bad steps first (the lowest k), then
 *                  (z, k, i, j) lexicographic"; clr_z_min is NaN with a bad step.  clr_z_at is (k, -1, -1) for a bad step and (0, -1, -1) if
 *                  clr_z is +inf throughout.
 *   eligible[B]    1 iff there is no bad step and clr_z_min >= z_tol (ints): the array ilqr_problem_select takes, so a multi-start can prefer the
 *                  starts that keep z_tol standard deviations from the cell.
 * `out` may be NULL; what it asks for is what ilqr_problem_closed_loop_cov returns, bit for bit per kernel, and the existing covariance entry
 * points return what they returned before.  The call changes nothing in the problem: plan, gains, multipliers, flags and obstacle terms stay as
 * they are; the obstacle terms a problem may hold play no part: the geometry is the call's.  The covariance kernels run as in
 * ilqr_problem_closed_loop_cov, with Sigma in a buffer of the context where the caller does not ask for it; k_cov_clr then reads xbar_k where
 * the plan lies and Sigma_k in its natural layout, lanes along the batch and one grid row per step, and k_cov_clr_fold folds a plan's steps in
 * ascending order on one lane.  Under ilqr_profile_enable the two are charged to ILQR_PROF_OTHER.
 * Refused, each with its own text: what ilqr_problem_closed_loop_cov refuses (a NULL `out` is not; B T n_x^2 >= 2^31 is refused whenever `clr`
 * asks for something, since Sigma is then formed); what the clearance calls refuse about robot, planes, obstacles, sets and the chain; a NaN
 * z_tol; clr and out both asking for nothing.
 * _dev: the arrays inside `out` and `clr` and world->obs are device pointers (the sigmas and the structs are read on the host before the call
 * returns); asynchronous on the context's stream, except that a call whose robot or chain differs from the previous call's waits for the stream
 * once, as the clearance calls do. */
typedef struct {
    double* clr_var;   /* [B][T] or NULL */
    double* clr_z;     /* [B][T] or NULL */
    double* clr_z_min; /* [B] or NULL */
    int*    clr_z_at;  /* [B][3] or NULL */
    int*    eligible;  /* [B] or NULL */
} ilqr_cl_cov_clr;
/* (the two prototypes stand behind ilqr_clr_robot and ilqr_clr_world, with the clearance calls) */

/* ---- multi-start: the calls that join instances (no reference function: the reference solves one problem from one U0) -------------------
 * iLQR is a local method; a caller with one task runs it from S starts on the idle lanes, keeps the best plan and polishes it.  Everything above
 * stays inside one instance; these four calls move data between instances, and between two problems, without leaving HBM.
 * Groups.  B = G * group_size; instance b = g * group_size + s is member s of group g.  Every call that takes a group_size fails with an error
 * text for group_size < 1 or B % group_size != 0.
 * _dev forms: every array is a device pointer and the call is asynchronous on the context's stream; structs are host memory, read before return.
 * Offsets: instance indices are ints; every offset into a device buffer or a natural-layout array is 64-bit (B T n may pass 2^31).
 * Under ilqr_profile_enable all of it is charged to ILQR_PROF_OTHER.
 *
 * ilqr_problem_adopt(dst, src, index, what): instance i of dst takes from instance index[i] of src (index[B_dst]) what the bits of `what` name:
 *   ILQR_ADOPT_STATE        q0, dq0
 *   ILQR_ADOPT_TARGETS      every keypoint's target
 *   ILQR_ADOPT_CONTROLS0    the controls src was given with ilqr_problem_set_controls (or adopted, spread or warm-started since): dst's U0
 *   ILQR_ADOPT_CONTROLS     the accepted plan's controls become dst's U0: the bytes ilqr_problem_get_U(src) returns.  src must hold a plan, as for
 *                           ilqr_problem_gains
 *   ILQR_ADOPT_MULTIPLIERS  src's current multipliers (ilqr_problem_get_lambda) become dst's current ones, not its lambda0
 *                           (ilqr_problem_reset_multipliers still restores what ilqr_problem_set_constraints gave dst); both problems must have
 *                           constraint rows of equal m and per_step
 * Both problems belong to one context, dst != src, and kind, nb_deriv, dof, horizon and n_kp are equal; every other descriptor field and the batch
 * sizes may differ, except that ILQR_ADOPT_TARGETS needs equal kp_joint flags (a joint-space keypoint's target is laid out as a state, a pose
 * keypoint's as f(x), and the rows are copied as they are).  Refused, each with its own text: a null problem or index, problems of two contexts, dst == src, a descriptor field of the five
 * that differs, TARGETS between keypoints whose kp_joint flags differ, `what` 0 or with an unknown bit, CONTROLS0 together with CONTROLS, STATE or CONTROLS0 from a src that was never given them, CONTROLS
 * without a plan, MULTIPLIERS without rows or with rows of another shape.  The host form refuses an index outside 0 .. B_src-1 and names the
 * first bad one; the _dev form cannot look: its kernel clamps every index into 0 .. B_src-1.  No out-of-range read is possible.
 * Copies are device to device between the private layouts (k_adopt_rows); a chain of fewer than 7 joints copies its padded rows as they are.
 * Afterwards dst is in the state the host setters would have left: start state / controls count as given, no plan and no gains (ilqr_problem_gains and
 * the closed-loop calls are refused until a solve).  src is untouched.  With index[b] = b / S the call replicates: a problem of G * S instances is
 * fed from a problem of G tasks.
 *
 * ilqr_problem_spread_controls(p, group_size, seeds): the starts of a group.  The member with global index member_offset + s = 0 keeps its U0;
 * every other member gets U0[b][k][i] += sigma_u[i] * z for k = 0 .. T-2 and the control entries i of the user's layout.
 *   z: the generator of ilqr_problem_closed_loop_noise above (Philox4x32-10, the same two normals per call); key = the seed, counter =
 *   (group_offset + g, member_offset + s, k, j); pair j serves control entries 2j and 2j + 1 (for an odd n_u the last z1 is dropped).
 *   The product is rounded on its own, then one rounded add.  An entry with sigma 0 is not touched, a pair with both sigmas 0 is not generated,
 *   the padded entries of a chain of fewer than 7 joints get nothing.  The draw of (seed, global group, global member, step, entry) depends on
 *   nothing else: a cut-out of groups or members, run with its offsets, reproduces the large call bit for bit.
 *   This is the stream of ilqr_problem_closed_loop_noise (there the counter is (instance, sample, step, pair)): a caller who draws both uses two seeds.
 * Needs controls set; afterwards the problem holds no plan and no gains.  Refused: a null seeds, a negative or non-finite sigma,
 * group_offset + G or member_offset + group_size beyond 2^32.  The two forms are one: the call takes no array and is asynchronous in both.
 *
 * ilqr_problem_select(p, group_size, score, eligible, winner, best, n_candidates): the best member of every group.
 *   score[B] or NULL (the cost ilqr_problem_get_cost returns); eligible[B] ints or NULL (all): e.g. formed from the `outcome` of a zero-noise,
 *   one-sample ilqr_problem_closed_loop_report(_con).
 *   Instance b is a candidate if eligible[b] != 0, its status carries neither ILQR_STATUS_NONFINITE nor ILQR_STATUS_SWEEP_IO and its score is finite.
 *   winner[G] (ints): the candidate of the group with the smallest score; scores compare as doubles (-0 ties with +0), ties go to the lowest b.
 *   best[G]: that score.  n_candidates[G] (ints): the number of candidates.
 *   A group without a candidate gets winner = g * group_size, best = NaN, n_candidates = 0: a winner is always a valid index for ilqr_problem_adopt.
 * Needs a plan (as ilqr_problem_gains).  Each output may be NULL, not all three.  The key (score, b) is totally ordered, so the result does not
 * depend on how the kernel maps groups to lanes (k_select_group: 1, 4, 16 or 64 lanes per group by group_size; any group_size).
 *
 * ilqr_problem_get_at(p, n, index, X, U, cost, iters, status): rows index[0 .. n-1] of what ilqr_problem_get_X, _get_U, _get_cost, _get_iters and
 * _get_status return, byte for byte: X[n][T][n_x], U[n][T-1][n_u], cost[n], iters[n], status[n].  Each output may be NULL, not all five; indices may
 * repeat and come in any order and are handled as in ilqr_problem_adopt (host form: refused outside 0 .. B-1; _dev: clamped).  n >= 1. */
#define ILQR_ADOPT_STATE 1
#define ILQR_ADOPT_TARGETS 2
#define ILQR_ADOPT_CONTROLS0 4
#define ILQR_ADOPT_CONTROLS 8
#define ILQR_ADOPT_MULTIPLIERS 16
typedef struct {
    unsigned long long seed;
    unsigned int group_offset, member_offset;   /* this call's first global group / member */
    double sigma_u[ILQR_MAX_NU];                /* user's control layout; 0 = none */
} ilqr_seeds;
int ilqr_problem_adopt(ilqr_problem* dst, ilqr_problem* src, const int* index, int what);
int ilqr_problem_adopt_dev(ilqr_problem* dst, ilqr_problem* src, const int* index, int what);
int ilqr_problem_spread_controls(ilqr_problem* p, int group_size, const ilqr_seeds* seeds);
int ilqr_problem_spread_controls_dev(ilqr_problem* p, int group_size, const ilqr_seeds* seeds);
int ilqr_problem_select(ilqr_problem* p, int group_size, const double* score, const int* eligible, int* winner, double* best, int* n_candidates);
int ilqr_problem_select_dev(ilqr_problem* p, int group_size, const double* score, const int* eligible, int* winner, double* best, int* n_candidates);
int ilqr_problem_get_at(ilqr_problem* p, int n, const int* index, double* X, double* U, double* cost, int* iters, int* status);
int ilqr_problem_get_at_dev(ilqr_problem* p, int n, const int* index, double* X, double* U, double* cost, int* iters, int* status);

/* ---- clearance: the distance of plans and executions from sphere obstacles and the planes of the cell (no reference function) ---------------
 * The geometric judgement of trajectories on the device: nothing is brought to the host, and no solver gets an obstacle term -- the calls score
 * trajectories that exist; choosing among starts with their `eligible` is a filter, not avoidance.  Clearance is judged at the T states of a
 * trajectory only: nothing is said about the motion between two steps (no swept volumes) or about any shape but spheres and half-spaces; the
 * robot against itself is judged on the self pairs the caller names (below), not on every pair of its spheres.  Under ilqr_profile_enable all of it is charged to ILQR_PROF_OTHER.
 *
 * Robot (ilqr_clr_robot): n_sph spheres, 1 .. ILQR_CLR_MAX_SPH.  Sphere i is carried by link sph_link[i], has the centre sph_c[i] in that link's
 *   frame and the radius sph_r[i] >= 0.  Link s in 0 .. n_seg-1 is the frame behind segment s of the descriptor's chain,
 *       F_s = F_{s-1} Trans(seg_xyz[s]) seg_R[s] Rot(seg_axis[s], q[seg_joint[s]])      (no rotation for a fixed segment), F_{-1} = I:
 *   link -1 is the base, link n_seg-1 the tool frame.  sph_link must be non-decreasing (the kernel advances a cursor along the chain).
 * Cell: n_planes half-spaces plane_n[l] . p >= plane_d[l], 0 .. ILQR_CLR_MAX_PLANES, shared by all trajectories; | |plane_n[l]| - 1 | <= 1e-9.
 * Obstacles (ilqr_clr_world): obs[n_sets][n_obs][4] = (cx, cy, cz, R) in the base frame; a slot with R < 0 is unused, so sets may hold different
 *   numbers.  Trajectory i belongs to set i / traj_per_set; n % traj_per_set == 0 and n_sets == n / traj_per_set (one world for all:
 *   traj_per_set = n).
 * Self pairs (n_self, 0 .. ILQR_CLR_MAX_SELF; a zeroed tail of the struct means none): self_pair[e] = (a, b) names two of the robot's own spheres
 *   with a < b and sph_link[a] < sph_link[b], and at least one moving segment s with sph_link[a] < s <= sph_link[b] (otherwise the pair's distance
 *   is a constant of the geometry).  The spheres that appear as a first member a are the anchors; at most ILQR_CLR_MAX_ANCHOR of them may be
 *   distinct (the walk keeps an anchor's centre until it reaches b, and the limit lets it do so in registers).  No pair may be given twice.
 * The clearance of a state is the minimum over the pairs (i, j) of
 *       (|p_i - o_j| - r_i) - R_j   for the active obstacle j < n_obs,          (n_l . p_i - d_l) - r_i   for plane l, j = n_obs + l,
 *       (|p_b - p_a| - r_b) - r_a   for the self pair (a, b), as the pair (i, j) = (b, n_obs + n_planes + a): the numbering continues the
 *                                   obstacles, then the planes, then the robot's own spheres; evaluated at sphere b behind b's obstacles and
 *                                   planes, the anchors ascending,
 *   p_i being the centre of sphere i in the base frame at the state's joint positions: the first dof entries of x in the user's layout, for every
 *   system kind and nb_deriv 1 and 2 (velocities and the time state play no part).  Ties go to the lowest i, then the lowest j.  Without an
 *   active obstacle, a plane or a self pair the clearance is +inf.  A step whose clearance is neither finite nor +inf is a bad step: one with a NaN
 *   or infinite position of a joint that moves a sphere (a joint at or before the last sphere's link; joints behind it are not read).
 * The clearance of a trajectory is the minimum over its steps k = 0 .. T-1 in the total order "bad steps first (the lowest k), then
 *   (clearance, k, i, j) lexicographic".  The order is total, so no result depends on how the kernels map steps to lanes.
 * Outputs (ilqr_clr_out; each may be NULL, not all):
 *   clr[n][T]       the clearance of every step, NaN on a bad step
 *   clr_min[n]      of the trajectory; NaN if it has a bad step
 *   clr_at[n][3]    (step, sphere, pair index j: obstacle, plane or own sphere as numbered above) of the minimum; (k, -1, -1) for a bad step; (0, -1, -1) if +inf throughout (ints)
 *   n_below[n]      the good steps with clearance < margin (strict; ints)
 *   eligible[n]     1 iff there is no bad step and clr_min >= margin: the array ilqr_problem_select takes (ints)
 *   stats[n / stats_group][ILQR_CLR_STATS] = { mean, min, n_hit, n_bad } over clr_min of the group's trajectories in index order: mean is the sum
 *                   over the good trajectories, added in ascending order with one rounding each, divided by their number; mean and min are NaN
 *                   if none is good; n_hit counts the good ones with clr_min < margin, n_bad those with a bad step.  Needs stats_group >= 1 and
 *                   n % stats_group == 0.
 * The structs are read before the call returns (host memory, both forms).  The _dev forms take device pointers for every array, obs included, and
 * are asynchronous on the context's stream; only a call whose robot or chain differs from the previous call's waits for the stream once, while it
 * replaces the geometry the kernels read.  Offsets into arrays are size_t (n T n_x may pass 2^31); a trajectory index is an int.
 *
 * ilqr_problem_clearance(p, robot, world, out): the plan the problem holds (the X ilqr_problem_get_X returns), n = B, read where it lies (the
 *   problem's own layout and buffer choice; nothing is copied out).  Needs a plan, as ilqr_problem_gains does, and changes nothing in the problem:
 *   plan, gains, multipliers and flags stay as they are.
 * ilqr_clearance_trajectories(ctx, desc, n, T, X, robot, world, out): any trajectories X[n][T][n_x] in the natural layout of desc
 *   (ilqr_dims_of), e.g. the X[B][S][T][n_x] of a closed-loop call with n = B S, traj_per_set = stats_group = S.  Of desc only kind, nb_deriv, dof
 *   and the chain are read.  Given the same states the two calls return the same bytes.
 * Refused, each with a text of its own: a null struct; n_sph outside 1 .. 32; a sph_link outside -1 .. n_seg-1 or a decreasing one; a negative or
 * non-finite radius, a non-finite centre; n_planes outside 0 .. 8, a non-unit or non-finite normal, a non-finite d; n_obs < 0 (or beyond 2^26 - 8, with self
 * pairs 2^26 - 8 - 32: the pair index shares an int with the sphere's), n_obs == 0 with no plane and no self pair, obs NULL with n_obs > 0; n_self
 * outside 0 .. 64, a self pair's index outside 0 .. n_sph-1, a >= b, the two spheres on one link or with no moving joint between, a repeated
 * pair, more than 8 distinct anchors; the set and stats divisibility rules; a NaN margin; all outputs NULL; stats with
 * stats_group < 1; a descriptor without a chain (n_seg < 1) or with a chain the lowering refuses; n < 1 or T < 1; no plan (problem form).  The host
 * forms also refuse a non-finite obstacle entry and name it. */
#define ILQR_CLR_MAX_SPH 32
#define ILQR_CLR_MAX_PLANES 8
#define ILQR_CLR_STATS 4
#define ILQR_CLR_MAX_SELF 64
#define ILQR_CLR_MAX_ANCHOR 8
typedef struct {
    int n_sph;
    int sph_link[ILQR_CLR_MAX_SPH];
    double sph_c[ILQR_CLR_MAX_SPH][3];
    double sph_r[ILQR_CLR_MAX_SPH];
    int n_planes;
    double plane_n[ILQR_CLR_MAX_PLANES][3];
    double plane_d[ILQR_CLR_MAX_PLANES];
    int n_self;
    int self_pair[ILQR_CLR_MAX_SELF][2];   /* (a, b): sphere indices */
} ilqr_clr_robot;
typedef struct {
    const double* obs;   /* [n_sets][n_obs][4] */
    int n_sets, n_obs, traj_per_set;
    double margin;
    int stats_group;     /* read only where stats is asked for */
} ilqr_clr_world;
typedef struct {
    double* clr;
    double* clr_min;
    int* clr_at;
    int* n_below;
    int* eligible;
    double* stats;
} ilqr_clr_out;
int ilqr_problem_clearance(ilqr_problem* p, const ilqr_clr_robot* robot, const ilqr_clr_world* world, const ilqr_clr_out* out);
int ilqr_problem_clearance_dev(ilqr_problem* p, const ilqr_clr_robot* robot, const ilqr_clr_world* world, const ilqr_clr_out* out);
int ilqr_clearance_trajectories(ilqr_ctx* ctx, const ilqr_problem_desc* desc, int n, int T, const double* X, const ilqr_clr_robot* robot,
                                const ilqr_clr_world* world, const ilqr_clr_out* out);
int ilqr_clearance_trajectories_dev(ilqr_ctx* ctx, const ilqr_problem_desc* desc, int n, int T, const double* X, const ilqr_clr_robot* robot,
                                    const ilqr_clr_world* world, const ilqr_clr_out* out);
/* "Analytic: ilqr_problem_closed_loop_cov_clr" above */
int ilqr_problem_closed_loop_cov_clr(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out,
                                     const ilqr_clr_robot* robot, const ilqr_clr_world* world, double z_tol, const ilqr_cl_cov_clr* clr);
int ilqr_problem_closed_loop_cov_clr_dev(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out,
                                         const ilqr_clr_robot* robot, const ilqr_clr_world* world, double z_tol, const ilqr_cl_cov_clr* clr);

/* ---- obstacle terms: a hinge penalty on clearance in the stage cost of the Riccati solvers (no reference function) ---------------------------
 * Avoidance, where the clearance calls above only judge: with these terms set, ilqr_solve_recursive, ilqr_solve_al, ilqr_problem_gains and
 * ilqr_problem_gains_al plan with a cost that grows as a sphere of the robot comes nearer than `margin` to an obstacle, a plane or the other
 * sphere of a self pair.  Every system
 * kind, nb_deriv 1 and 2, chains of 1 to 7 joints.  Robot, planes, obstacle sets and the pair clearances
 *       clr_ij(q) = (|p_i - o_j| - r_i) - R_j   (active obstacle j),          (n_l . p_i - d_l) - r_i   (plane l, j = n_obs + l)
 * and, for every self pair (a, b) of the robot,   clr_ab(q) = (|p_b - p_a| - r_b) - r_a,
 * are exactly those of "clearance"; q is the first dof entries of x in the user's layout.  With the activation distance margin = world->margin
 * and the weight w >= 0, at every step k = 0 .. T-1 (the terminal state included, as for the limit terms):
 *       h_ij   = max(0, margin - clr_ij(q_k))                  every pair (i, j): the active obstacles of the instance's set, then the planes
 *       c_obs  = w * sum_ij h_ij^2                             joins the stage cost: cost, trace, line search, ilqr_problem_get_cost
 *       l_x   += -w * sum_ij h_ij grad_ij                      joint-position entries only
 *       l_xx  +=  w * sum_{ij : h_ij > 0} grad_ij grad_ij'     Gauss-Newton; the joint-position block only
 *       grad_ij = n_ij' Jp_i(q),   n_ij = (p_i - o_j) / |p_i - o_j| for an obstacle, plane_n[l] for a plane;
 *   Jp_i is the position Jacobian of sphere centre i: column m is a_m x (p_i - r_m), a_m and r_m the axis and origin of joint m in the base
 *   frame, for the joints m that move link sph_link[i], and 0 for the others.  This is the reference's keypoint convention (cost = e'Qe,
 *   l_x = -J'Qe, l_xx = J'QJ; System.cpp:248-308) for a one-sided scalar keypoint on clearance with target `margin` and precision w: l_x is
 *   half the gradient of the cost, as for every other term.  The exact Hessian's term h_ij grad^2 clr_ij is left out.
 *   A self pair (a, b) is one more term of the sums, h_ab = max(0, margin - clr_ab) with the same margin and weight, added at sphere b behind b's
 *   planes, the anchors ascending.  Its normal is n_ab = (p_b - p_a) / |p_b - p_a| and grad_ab[m] = n_ab . (a_m x (p_b - r_m)) for the joints m that
 *   move b's link but not a's; it is exactly 0 for every other joint: a joint that moves both spheres moves them rigidly, its column
 *   a_m x (p_b - p_a) is orthogonal to n_ab, and the library writes that 0 -- it does not compute and cancel.  Coincident centres add their cost
 *   and a zero gradient, as for an obstacle.
 *   A pair with p_i == o_j exactly adds its cost and a zero gradient.  Velocity, time and control entries get nothing, nor do the padded joints of
 *   a chain of fewer than 7 joints.  The sum runs over ALL pairs, not only the nearest, so the cost is C1 in q.  Summation order: spheres
 *   ascending; per sphere the obstacles ascending, then the planes, then the self pairs whose b it is; one rounding per operation (no contraction), and the weight multiplies the
 *   finished sums.  A stage's terms are added as the limit terms are: behind the keypoint or first limit set's terms, before the second limit
 *   set's; the stage's cost (system part + c_obs) is formed first and then joins the running sum.  One per-state function serves the solvers'
 *   rollouts, their derivative pass and the query below: the same state gives the same cost bits everywhere.  A state with a NaN or infinite
 *   position of a joint that moves a sphere gives a NaN cost (status ILQR_STATUS_NONFINITE by the usual rule).
 *
 * ilqr_problem_set_obstacles(p, robot, world, weight): instance b reads set b / traj_per_set (n = B in the rules of "clearance"); stats_group is
 *   not read.  Everything is copied into memory the problem owns before the call returns: no pointer is kept (_dev: world->obs is a device
 *   pointer and the copy is device to device; the structs are host memory in both forms).  robot == NULL removes the terms, and the problem is
 *   then planned exactly as before.  A setter: afterwards the problem holds no plan and no gains.  Problems with obstacle terms run on the generic
 *   lane-per-instance kernel set, whatever the pins say (as a second limit set and shared keypoint steps do): they pay that set's price --
 *   unless ilqr_ctx_set_obstacle_path (below) sends them to the cooperative kernels.
 *   Refused, each with its own text: what the clearance calls refuse about robot, planes, obstacles, sets and the chain; a negative or non-finite
 *   weight; a NaN or infinite margin.  ilqr_solve_batch_cp and ilqr_solve_batch refuse a problem that has obstacle terms.
 * ilqr_problem_obstacle_terms(p, cost, lx, lxx): the terms at the plan the problem holds (needs one, as ilqr_problem_gains does): cost[B][T],
 *   lx[B][T][dof], lxx[B][T][dof][dof] (the full symmetric matrix, mirrored from one triangle); each may be NULL, not all.  Changes nothing in
 *   the problem.  _dev: device pointers, asynchronous on the context's stream.
 * The closed-loop calls (ilqr_problem_closed_loop*) do NOT add the obstacle term: their costs stay the system's stage cost.  Executions are
 *   scored with ilqr_clearance_trajectories. */
int ilqr_problem_set_obstacles(ilqr_problem* p, const ilqr_clr_robot* robot, const ilqr_clr_world* world, double weight);
int ilqr_problem_set_obstacles_dev(ilqr_problem* p, const ilqr_clr_robot* robot, const ilqr_clr_world* world, double weight);
int ilqr_problem_obstacle_terms(ilqr_problem* p, double* cost, double* lx, double* lxx);
int ilqr_problem_obstacle_terms_dev(ilqr_problem* p, double* cost, double* lx, double* lxx);
/* The kernel path of a problem with obstacle terms: context state of its own (ilqr_ctx_set_crosscheck does not touch it; no environment variable),
 * in force for every later solve and gains call on the context.  ILQR_OBSTACLE_PATH_GENERIC (the default): the generic lane-per-instance set, as
 * described above.  ILQR_OBSTACLE_PATH_COOPERATIVE: the cooperative kernels of the single-integrator systems, where all of this holds: PosOrn or
 * JointSpace with nb_deriv 1, at most 16 step sizes, no AL rows or at most 4 shared rows on the state alone, no second limit set, no keypoints
 * that share a timestep, arrays addressable with 32-bit offsets, and generic_kernels not pinned (that pin wins).  Every other problem, and every
 * problem without obstacle terms, is planned and solved exactly as under GENERIC.  The term's definition does not depend on the path; the two
 * paths agree to rounding, not bit for bit.  On the cooperative path a stage's l_x, l_xx are formed in one fixed order before the sweep reads
 * them -- the keypoint's entry (limits in it) at a keypoint step, the limit terms at any other, and the obstacle terms added to that --; the
 * line search's cost of step size alpha is (task cost at the keypoints + limit cost) + sum_k c_obs(x(alpha)_k), the inner sum over the steps in
 * ascending k, whatever the batch size, traj_per_set or the forward pin, with x(alpha) = fma(alpha, x(1) - xbar, xbar) (x(1) itself at alpha = 1),
 * the expression that forms the accepted plan; the initial trajectory's cost is (system cost) + that sum at xbar.  A NaN position gives a NaN sum.
 * Any other value of `path` is refused with a text. */
#define ILQR_OBSTACLE_PATH_GENERIC 0
#define ILQR_OBSTACLE_PATH_COOPERATIVE 1
int ilqr_ctx_set_obstacle_path(ilqr_ctx* ctx, int path);

/* ---- stand-alone batched kinematics: KDLRobot::updateKinematics for n configurations ---------------------- */
/* (src/sim/KDLRobot.cpp:83-115): q[n][dof] (dq[n][dof] or NULL) -> pos[n][3], quat[n][4] (w,x,y,z), jac[n][6][dof];
 * any output may be NULL.  Host pointers. */
int ilqr_fk_batch(ilqr_ctx* ctx, const ilqr_problem_desc* desc, int n, const double* q, double* pos, double* quat, double* jac);

/* ---- batched linear-quadratic tracking: solver::LQT (include/ilqr_planner/solver/lqt.h:23-86, src/solver/lqt.cpp) -------------------------
 * B instances of LQT(A, B, Qs, states, rfactor, nb_deriv) that share A, B, R = r I and either share the precisions Qs (one Riccati chain for the
 * batch, qs_per_instance = 0) or carry their own (one chain per instance).  n = n_x, m = n_u, N = number of targets.  Shapes (natural layout):
 * A[n][n], Bm[n][m], Qs[N][n][n] shared or Qs[B][N][n][n] per instance, Qs[N-1] being the terminal weight P_{N-1} of the DP form (the reference's
 * solveDP takes Qs.back() there, solveLinAl Qs[N-1]: a caller with more than N matrices passes the one it wants).  r is the R diagonal value
 * (the reference's pow(float rfactor, nb_deriv) belongs to the caller).  Precisions are symmetric: Q enters as (Q + Q') / 2.
 * Limits: 1 <= n <= ILQR_LQT_MAX_NX, 1 <= m <= ILQR_LQT_MAX_NU, N >= 1; beyond them creation fails with an error text naming the range.
 * A handle belongs to its context: ilqr_ctx_destroy frees it (the caller's pointer becomes invalid).  No result depends on the batch size. */
#define ILQR_LQT_MAX_NX 16
#define ILQR_LQT_MAX_NU 8
typedef struct ilqr_lqt ilqr_lqt;
/* lqt.cpp:16-25 (the constructor) */
int ilqr_lqt_create(ilqr_ctx* ctx, int n_x, int n_u, int N, int batch, const double* A, const double* Bm, double r, const double* Qs,
                    int qs_per_instance, ilqr_lqt** out);
void ilqr_lqt_destroy(ilqr_lqt* h);
/* the constructor's `states`: mu[B][N][n_x] (target t of instance b at mu[b][t]); invalidates earlier solves */
int ilqr_lqt_set_targets(ilqr_lqt* h, const double* mu);
int ilqr_lqt_set_targets_dev(ilqr_lqt* h, const double* mu);
/* solveDP (lqt.cpp:29-53): P_t, d_t for t = N-1 .. 0; asynchronous on the context's stream */
int ilqr_lqt_solve_dp(ilqr_lqt* h);
/* solveLinAl (lqt.cpp:55-89): the minimiser of the tracking cost from x_0 = mu_0, computed by the Riccati recursion and a forward rollout (the
 * dense normal equations are never formed; the minimiser is unique, so the two agree to rounding times the problem's conditioning).  Runs
 * ilqr_lqt_solve_dp first if it has not run on the current targets. */
int ilqr_lqt_solve_lin_al(ilqr_lqt* h);
/* getCommand(t, x) (lqt.cpp:102-120): x[B][n_x] -> u[B][n_u], the reference's law at tau = t + 1; t in -1 .. N-2.
 * Fails with "solveDP() first" before ilqr_lqt_solve_dp. */
int ilqr_lqt_command(ilqr_lqt* h, int t, const double* x, double* u);
int ilqr_lqt_command_dev(ilqr_lqt* h, int t, const double* x, double* u);
/* results; before the solve that makes them they fail with "solveLinal() or solveQP() first" (U, X) or "solveDP() first" (P, d) */
int ilqr_lqt_get_U(ilqr_lqt* h, double* U);      /* [B][N-1][n_u]  u of solveLinAl, getCommand(t) = U[b][t] */
int ilqr_lqt_get_U_dev(ilqr_lqt* h, double* U);
int ilqr_lqt_get_X(ilqr_lqt* h, double* X);      /* [B][N][n_x]    getPredictedStates (lqt.cpp:122-127), x_0 = mu_0 first */
int ilqr_lqt_get_X_dev(ilqr_lqt* h, double* X);
int ilqr_lqt_get_P(ilqr_lqt* h, double* P);      /* [N][n_x][n_x] shared, [B][N][n_x][n_x] per instance: the reference's Ps */
int ilqr_lqt_get_d(ilqr_lqt* h, double* d);      /* [B][N][n_x]    the reference's ds */

/* ---- instrumentation ----------------------------------------------------------------------------------------- */
/* When enabled, every kernel launch is bracketed by hipEvents on the launch stream; totals are read back with
 * ilqr_profile_get (index: ILQR_PROF_*).  Used by bench.py for the roofline figures. */
#define ILQR_PROF_ROLLOUT 0
#define ILQR_PROF_BACKWARD 1
#define ILQR_PROF_FORWARD 2
#define ILQR_PROF_OTHER 3
#define ILQR_PROF_APPLY 4 /* second forward pass: re-roll of the winning step size */
#define ILQR_PROF_COUNT 5
int ilqr_profile_enable(ilqr_ctx* ctx, int on);
int ilqr_profile_reset(ilqr_ctx* ctx);
int ilqr_profile_get(ilqr_ctx* ctx, int which, double* total_ms, int* launches);

#ifdef __cplusplus
}
#endif
#endif
