// ilqr_capi.cpp -- implementation of the C ABI declared in include/ilqr_hip.h (compiled with hipcc).
//
// Host-side orchestration only: lowering of the POD problem description to the device descriptor, buffer
// ownership, layout conversion at the boundary and the per-iteration launch sequence
//   init rollout -> nb_iter x { backward sweep, forward line search }
// which mirrors ILQRRecursive::solve / AL_ILQR::solve (reference src/solver/ILQRRecursive.cpp:21-181,
// src/solver/AL-ILQR.cpp:50-232).  No CPU fallback exists: every entry point fails loudly if HIP does.
// The one exception to "host-side only": the small kernels that join instances (ilqr_multistart_kernels.hpp, included at the end) are compiled
// with this file, for the reason given there; the clearance kernels (ilqr_clearance_kernels.hpp) and those of the obstacle terms' cooperative path
// (ilqr_obstacle_coop_kernels.hpp) likewise.
#include "../../include/ilqr_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ilqr_batchcp.hpp"
#include "ilqr_clearance.hpp"
#include "ilqr_closed_loop.hpp"
#include "ilqr_closed_loop_cov.hpp"
#include "ilqr_ctx.hpp"
#include "ilqr_kernels.hpp"
#include "ilqr_multistart.hpp"
#include "ilqr_obstacle.hpp"
#include "ilqr_plan.hpp"

using namespace ilqr;

// A device buffer of doubles that only grows: the staging area and the workspaces of the closed loop.  A call whose need is covered allocates nothing.
struct DevScratch {
    double* ptr = nullptr;
    size_t elems = 0;
    int reserve(ilqr_ctx* c, size_t n) {
        if (elems >= n) return 0;
        if (ptr) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(ptr)); ptr = nullptr; elems = 0; }  // kernels in flight may still read it
        HIPCHK(c, hipMalloc((void**)&ptr, n * sizeof(double)));
        elems = n;
        return 0;
    }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; elems = 0; }
};

struct ilqr_problem {
    ilqr_ctx* ctx = nullptr;
    ilqr_problem_desc desc;  // as given: the user's dof
    ilqr_dims udims;         // the user's dimensions: every array crossing the ABI
    ilqr_dims dims;          // the device's (7 joints): every device buffer
    DofMap map;              // user index -> device index (ilqr_dofmap.hpp)
    bool mapped = false;     // dof < 7: the layout conversions go through `map`; a 7-joint problem takes the plain ones
    IndexMap qmap;           // q0 / dq0: [dof] -> [7]
    int B = 0, Bp = 0, T = 0;
    DevDesc hdesc;
    DevDesc* ddesc = nullptr;
    DevDesc* ddesc_half[2] = {nullptr, nullptr};  // the descriptor with B = the half's instance count (split solves)
    int half_b0[2] = {0, 0}, half_B[2] = {0, 0};
    Bufs bufs;
    std::vector<void*> allocs;
    double *conA = nullptr, *conb = nullptr;  // device copies of the shared constraint rows
    double* lambda0 = nullptr;                // initial multipliers, kept for ilqr_problem_reset_multipliers
    bool con_state_only = false;              // no constraint row touches the controls (enables the closed-form sweep)
    int trace_iters = 0;
    DevScratch staging;  // device staging for host<->device natural-layout transfers
    int last_nb_iter = 0;
    bool has_controls = false, has_state = false;
    bool has_gains = false;  // a Riccati solve with nb_iter >= 1 or ilqr_problem_gains has run since the inputs last changed: X, U, KD are one plan (closed_loop)
    bool has_plan = false;   // one of the four solvers has run since the inputs last changed: X, U are a plan ilqr_problem_gains can sweep about
    DevScratch cl_cost;  // closed_loop_noise without a cost array: the per-sample costs k_closed_loop_stats reduces
    DevScratch cl_kpx;   // closed_loop: state | control of every sample at the step-table entries (k_closed_loop_coop -> k_closed_loop_kp)
    DevScratch cl_rep;   // closed_loop_report through device pointers: kp_err | lim_cost where the caller asks only for their reductions
    DevScratch cl_con_ws;   // closed_loop_report_con through device pointers: con_max | con_steps where the caller asks only for their reductions
    DevScratch cl_cov_ws;   // closed_loop_cov: the per-lane matrices of the generic kernel k_cl_cov
    DevScratch cl_cov_kps;  // closed_loop_cov through device pointers: kp_Sigma where the caller asks only for kp_var
    DevScratch ms_idx;   // adopt / get_at / select through host pointers: the index (or the eligibility flags) as ints
    DevScratch ms_out;   // select / get_at through host pointers: best | winner, n_candidates and iters | status as ints
    // obstacle terms of the stage cost (ilqr_problem_set_obstacles): the geometry, the obstacle sets and the slots of k_obs_derivs are device
    // memory of this problem; `obs` is what the kernels are given.  Problems with these terms run on the generic kernels unless the context's
    // obstacle path sends them to the cooperative ones (plan_input).
    bool has_obs = false;
    ObsProblem obs = {};
    size_t obs_sets_bytes = 0;
    // the cooperative path of these terms (RiccatiPlan::obs_dense), allocated at its first solve: l_x | l_xx of every stage (one kpd entry per
    // step) and the obstacle cost of every (step, step size) of a line search
    ObsDense obs_dense = {};
    bool u0_zero = false;  // the initial controls given from the host are all zero (lets the wide-basis batch solver skip their projection)
    BatchCPState cp;
    BatchWideState cpw;
};

// ------------------------------------------------------------------------------------------------ misc

extern "C" const char* ilqr_version(void) { return "ilqr_hip 0.1 (gfx950, fp64)"; }

extern "C" void ilqr_desc_defaults(ilqr_problem_desc* d) {
    std::memset(d, 0, sizeof(*d));
    d->reg = 1e-6;
    d->alpha_floor = 1e-3;
    d->stop_tol = 1e-3;
    d->nb_deriv = 1;
    d->dof = 7;
}

extern "C" int ilqr_dims_of(const ilqr_problem_desc* d, ilqr_dims* o) {
    if (!d || !o) return 1;
    if (d->kind != ILQR_SYS_POS_ORN && d->kind != ILQR_SYS_POS_ORN_TIME && d->kind != ILQR_SYS_JOINT && d->kind != ILQR_SYS_JOINT_TIME) return 1;
    if (d->nb_deriv != 1 && d->nb_deriv != 2) return 1;
    if (d->kind == ILQR_SYS_JOINT || d->kind == ILQR_SYS_JOINT_TIME) {  // JointSpace(Time)PlannerSys localInit; 2nd order inconsistent upstream
        if (d->nb_deriv != 1) return 1;
        o->n_x = o->n_u = o->n_f = o->n_Q = d->dof + (d->kind == ILQR_SYS_JOINT_TIME ? 1 : 0);
        return 0;
    }
    const int tm = d->kind == ILQR_SYS_POS_ORN_TIME ? 1 : 0;
    o->n_x = d->nb_deriv * d->dof + tm;  // PosOrnPlannerSys.cpp:74 / PosOrnTimePlannerSys.cpp:67
    o->n_u = d->dof + tm;
    o->n_f = 7 * d->nb_deriv + tm;
    o->n_Q = o->n_f - d->nb_deriv;
    return 0;
}

extern "C" int ilqr_ctx_create(int device_id, ilqr_ctx** out) {
    if (!out) return 1;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return 2;  // no HIP device: fail loudly, there is no CPU path
    if (device_id < 0 || device_id >= n) return 3;
    if (hipSetDevice(device_id) != hipSuccess) return 4;
    auto* c = new ilqr_ctx();
    c->device = device_id;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return 5;
    }
    c->stream = c->own_stream;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && cus > 0) c->n_simd = 4 * cus; }
    *out = c;
    return 0;
}

static void clr_release(ilqr_ctx* c);  // the clearance calls' buffers (below)

extern "C" void ilqr_ctx_destroy(ilqr_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    while (!c->problems.empty()) ilqr_problem_destroy(c->problems.back());  // handles held by the caller become invalid
    while (!c->cleanups.empty()) { const auto cl = c->cleanups.back(); cl.destroy(cl.handle); }  // each destroy removes its own entry
    (void)hipStreamSynchronize(c->stream);
    clr_release(c);
    for (auto& p : c->pending) (void)hipEventDestroy(p.a);
    for (auto e : c->pool) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; i++) {
        if (c->half_stream[i]) (void)hipStreamSynchronize(c->half_stream[i]);
        if (c->half_stream[i]) (void)hipStreamDestroy(c->half_stream[i]);
        if (c->ev_half_done[i]) (void)hipEventDestroy(c->ev_half_done[i]);
    }
    if (c->ev_begin) (void)hipEventDestroy(c->ev_begin);
    if (c->ev_stagger) (void)hipEventDestroy(c->ev_stagger);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

extern "C" const char* ilqr_last_error(const ilqr_ctx* c) { return c ? c->err.c_str() : "null context"; }

extern "C" int ilqr_ctx_set_stream(ilqr_ctx* c, void* s) {
    if (!c) return 1;
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return 0;
}

extern "C" int ilqr_ctx_set_split(ilqr_ctx* c, int on) {
    if (!c) return 1;
    if (on < 0 || on > 2) return fail(c, "ilqr_ctx_set_split: mode must be 0, 1 or 2 (got " + std::to_string(on) + ")");
    c->split = on;
    return 0;
}

static_assert((int)SweepPin::Mfma == ILQR_XC_SWEEP_MFMA && (int)SweepPin::Rows == ILQR_XC_SWEEP_ROWS && (int)SweepPin::SiWave == ILQR_XC_SWEEP_SI_WAVE &&
              (int)SweepPin::SiWg == ILQR_XC_SWEEP_SI_WG && (int)SweepPin::SiWgIo == ILQR_XC_SWEEP_SI_WG_IO && (int)SweepPin::SiWgPrep == ILQR_XC_SWEEP_SI_WG_PREP && (int)FwdPin::Wg == ILQR_XC_FWD_WG &&
              (int)FwdPin::Dpp == ILQR_XC_FWD_DPP && (int)FwdPin::WgLds == ILQR_XC_FWD_WG_LDS && (int)FwdPin::WgIo == ILQR_XC_FWD_WG_IO && (int)RerollPin::Rows == ILQR_XC_REROLL_ROWS && (int)RerollPin::Dpp == ILQR_XC_REROLL_DPP,
              "variant pins of ilqr_plan.hpp and include/ilqr_hip.h");

extern "C" int ilqr_ctx_set_crosscheck(ilqr_ctx* c, int generic_kernels, int cp_lane_solve, int cp_general, int sweep, int forward, int reroll) {
    if (!c) return 1;
    if (sweep < 0 || sweep > 7 || sweep == 3) return fail(c, "ilqr_ctx_set_crosscheck: sweep must be ILQR_XC_AUTO, ILQR_XC_SWEEP_MFMA, ILQR_XC_SWEEP_ROWS, ILQR_XC_SWEEP_SI_WAVE, ILQR_XC_SWEEP_SI_WG, ILQR_XC_SWEEP_SI_WG_IO or ILQR_XC_SWEEP_SI_WG_PREP");
    if (forward < 0 || forward > 4) return fail(c, "ilqr_ctx_set_crosscheck: forward must be ILQR_XC_AUTO, ILQR_XC_FWD_WG, ILQR_XC_FWD_DPP, ILQR_XC_FWD_WG_LDS or ILQR_XC_FWD_WG_IO");
    if (reroll < 0 || reroll > 2) return fail(c, "ilqr_ctx_set_crosscheck: reroll must be ILQR_XC_AUTO, ILQR_XC_REROLL_ROWS or ILQR_XC_REROLL_DPP");
    c->xc_sweep = (SweepPin)sweep;
    c->xc_forward = (FwdPin)forward;
    c->xc_reroll = (RerollPin)reroll;
    c->xc_generic = generic_kernels != 0;
    c->xc_cp_lane = cp_lane_solve != 0;
    c->xc_cp_general = cp_general != 0;
    return 0;
}

extern "C" int ilqr_ctx_set_obstacle_path(ilqr_ctx* c, int path) {
    if (!c) return 1;
    if (path != ILQR_OBSTACLE_PATH_GENERIC && path != ILQR_OBSTACLE_PATH_COOPERATIVE)
        return fail(c, "ilqr_ctx_set_obstacle_path: path must be ILQR_OBSTACLE_PATH_GENERIC (0) or ILQR_OBSTACLE_PATH_COOPERATIVE (1) (got " + std::to_string(path) + ")");
    c->obs_coop = path == ILQR_OBSTACLE_PATH_COOPERATIVE;
    return 0;
}

extern "C" int ilqr_ctx_synchronize(ilqr_ctx* c) {
    if (!c) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------ profiling

static hipEvent_t ev_get(ilqr_ctx* c) {
    if (!c->pool.empty()) {
        hipEvent_t e = c->pool.back();
        c->pool.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
// One event is recorded in FRONT of every kernel launch (and one behind the last launch of a solve): the interval between two
// consecutive marks is charged to the kernel that the first one precedes.  Half the events of a start/stop pair per kernel.
static void prof_collect(ilqr_ctx* c) {
    if (c->pending.empty()) return;
    (void)hipStreamSynchronize(c->stream);
    for (size_t i = 0; i + 1 < c->pending.size(); i++) {
        const auto& p = c->pending[i];
        float ms = 0;
        if (p.which >= 0 && hipEventElapsedTime(&ms, p.a, c->pending[i + 1].a) == hipSuccess) {
            c->prof_ms[p.which] += ms;
            c->prof_n[p.which] += 1;
        }
    }
    for (auto& p : c->pending) c->pool.push_back(p.a);
    c->pending.clear();
}
static void prof_mark(ilqr_ctx* c, int which) {  // which < 0: end mark (closes the previous interval, charges nothing itself)
    if (!c->profile) return;
    hipEvent_t e = ev_get(c);
    (void)hipEventRecord(e, c->stream);
    c->pending.push_back({e, nullptr, which});
    if (which < 0 && c->pending.size() > 4096) prof_collect(c);  // synchronises; only with profiling on and only every few hundred solves
}
struct ProfScope {  // marks the launch that follows; the interval is closed by the next mark
    ProfScope(ilqr_ctx* c, int w) { prof_mark(c, w); }
};

static void prof_hook_fn(void* c, int which) { prof_mark((ilqr_ctx*)c, which); }
static ilqr::ProfHook prof_hook(ilqr_ctx* c) {
    ilqr::ProfHook h;
    if (c->profile) { h.mark = prof_hook_fn; h.ctx = c; }
    return h;
}

extern "C" int ilqr_profile_enable(ilqr_ctx* c, int on) {
    if (!c) return 1;
    prof_collect(c);
    c->profile = on != 0;
    return 0;
}
extern "C" int ilqr_profile_reset(ilqr_ctx* c) {
    if (!c) return 1;
    prof_collect(c);
    for (int i = 0; i < ILQR_PROF_COUNT; i++) { c->prof_ms[i] = 0; c->prof_n[i] = 0; }
    return 0;
}
extern "C" int ilqr_profile_get(ilqr_ctx* c, int which, double* ms, int* n) {
    if (!c || which < 0 || which >= ILQR_PROF_COUNT) return 1;
    prof_collect(c);
    if (ms) *ms = c->prof_ms[which];
    if (n) *n = c->prof_n[which];
    return 0;
}

// ------------------------------------------------------------------------------------------------ lowering

static void mat3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

static_assert(DOF == DEV_DOF, "ilqr_dofmap.hpp and ilqr_device.hpp");
static_assert(STEP_MAX_KP == ILQR_MAX_KP && MAX_KP == ILQR_MAX_KP, "ilqr_steps.hpp, ilqr_device.hpp and include/ilqr_hip.h");

static int check_dof(ilqr_ctx* c, int dof) {
    if (dof < 1 || dof > DOF) return fail(c, "chains of 1 to 7 moving joints are supported (dof = " + std::to_string(dof) + ")");
    return 0;
}

// Fold runs of fixed segments into the following joint's pre-transform; the rest becomes the tail.  A chain of dof < 7 joints gets 7 - dof
// inert joints behind its last one (identity pre-transform, zero offset, zero axis; ilqr_dofmap.hpp): at q = 0 they are the identity exactly.
static int lower_chain(ilqr_ctx* c, const ilqr_problem_desc& d, DevChain& ch) {
    if (check_dof(c, d.dof)) return 1;
    if (d.n_seg < 1 || d.n_seg > ILQR_MAX_SEG) return fail(c, "bad n_seg");
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    int nj = 0;
    for (int s = 0; s < d.n_seg; s++) {
        double Rn[9];
        for (int i = 0; i < 3; i++) p[i] += R[3 * i] * d.seg_xyz[s][0] + R[3 * i + 1] * d.seg_xyz[s][1] + R[3 * i + 2] * d.seg_xyz[s][2];
        mat3(R, d.seg_R[s], Rn);
        std::memcpy(R, Rn, sizeof(R));
        const int j = d.seg_joint[s];
        if (j >= 0) {
            if (j != nj) return fail(c, "moving joints must be numbered 0..dof-1 in chain order");
            if (nj >= DOF) return fail(c, "chain has more than 7 moving joints (chains of 1 to 7 moving joints are supported)");
            std::memcpy(ch.Rpre[nj], R, sizeof(R));
            std::memcpy(ch.ppre[nj], p, sizeof(p));
            std::memcpy(ch.axis[nj], d.seg_axis[s], 3 * sizeof(double));
            nj++;
            const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            std::memcpy(R, I, sizeof(R));
            p[0] = p[1] = p[2] = 0;
        }
    }
    if (nj != d.dof)
        return fail(c, "chain has " + std::to_string(nj) + " moving joints, descriptor says " + std::to_string(d.dof) + " (chains of 1 to 7 moving joints are supported)");
    for (int j = nj; j < DOF; j++) {
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        std::memcpy(ch.Rpre[j], I, sizeof(I));
        for (int i = 0; i < 3; i++) ch.ppre[j][i] = ch.axis[j][i] = 0.0;
    }
    std::memcpy(ch.Rtail, R, sizeof(R));
    std::memcpy(ch.ptail, p, sizeof(p));
    return 0;
}

// Every per-joint field goes through the map m (identity for 7 joints): padded control weights are the first joint's (a uniform R stays
// uniform, so plan_riccati decides as for 7 joints), padded limits and precisions are 0.
static int lower_desc(ilqr_ctx* c, const ilqr_problem_desc& d, const DofMap& m, int B, int Bp, DevDesc& h) {
    ilqr_dims dm;
    if (ilqr_dims_of(&d, &dm)) return fail(c, "unsupported system kind / nb_deriv");
    const IndexMap &mx = m.x, &mu = m.u;
    auto xs = [&](const double* v, int j) { return mx.usr[j] < 0 ? 0.0 : v[mx.usr[j]]; };
    auto xi = [&](const int* v, int j) { return mx.usr[j] < 0 ? 0 : v[mx.usr[j]]; };
    auto us = [&](const double* v, int j) { return v[mu.usr[j] < 0 ? 0 : mu.usr[j]]; };
    std::memset(&h, 0, sizeof(h));
    if (!((d.kind == ILQR_SYS_JOINT || d.kind == ILQR_SYS_JOINT_TIME) && d.n_seg == 0) && lower_chain(c, d, h.chain)) return 1;  // joint-space systems need no chain
    if (d.horizon < 2) return fail(c, "horizon must be >= 2");
    h.kind = d.kind; h.nd = d.nb_deriv; h.T = d.horizon; h.B = B; h.Bp = Bp; h.dt = d.dt;
    for (int j = 0; j < mu.n_dev; j++) h.R_diag[j] = us(d.R_diag, j);
    {   // SequentialSystem: every sub-system adds the limit terms once -- q'Lq and L'q scale with the multiplicity, L'L too
        const double mult = d.limit_multiplicity > 1 ? (double)d.limit_multiplicity : 1.0;
        h.limits_set = d.limits_set;
        h.penalty = d.penalty * mult;
        h.pen_xx = d.penalty * d.penalty * mult;
        h.batch_limits = (d.limit_multiplicity > 1 || d.is_sequence) ? 0 : 1;
        h.lim2 = d.limits2_set ? 1 : 0;
        if (d.limits2_set) {
            const double mult2 = d.limit_multiplicity2 > 1 ? (double)d.limit_multiplicity2 : 1.0;
            h.penalty2 = d.penalty2 * mult2;
            h.pen_xx2 = d.penalty2 * d.penalty2 * mult2;
            for (int j = 0; j < mx.n_dev; j++) { h.smax2[j] = xs(d.state_max2, j); h.smin2[j] = xs(d.state_min2, j); h.lw2[j] = xi(d.limit_weight2, j); }
        }
    }
    for (int j = 0; j < mx.n_dev; j++) { h.smax[j] = xs(d.state_max, j); h.smin[j] = xs(d.state_min, j); h.lw[j] = xi(d.limit_weight, j); }
    if (d.n_kp < 0 || d.n_kp > ILQR_MAX_KP) return fail(c, "bad n_kp");
    h.n_kp = d.n_kp;
    for (int k = 0; k < d.n_kp; k++) {
        if (d.kp_timestep[k] < 0 || d.kp_timestep[k] >= d.horizon) return fail(c, "keypoint timestep outside the horizon");
        if (k > 0 && d.kp_timestep[k] < d.kp_timestep[k - 1]) return fail(c, "keypoint timesteps must be non-decreasing");
        // a plain System keeps one keypoint per step (System.cpp:78-80): only the sub-systems of a sequence put several on one step
        if (k > 0 && d.kp_timestep[k] == d.kp_timestep[k - 1] && !d.is_sequence && d.limit_multiplicity <= 1)
            return fail(c, "keypoint timesteps must be unique and ascending unless is_sequence = 1 (the keypoints of a SequentialSystem's sub-systems may share a step)");
        h.kp_t[k] = d.kp_timestep[k];
        if (d.kp_joint[k] && !((d.kind == ILQR_SYS_POS_ORN || d.kind == ILQR_SYS_POS_ORN_TIME) && d.nb_deriv == 1))
            return fail(c, "kp_joint is for PosOrn / PosOrnTime systems with nb_deriv = 1 (a joint-space system needs no flag)");
        if (d.kp_joint[k] && (d.kp_dist[k] || d.kp_has_frame[k])) return fail(c, "a joint-space keypoint has no dead zone and no object frame");
        h.kp_joint[k] = d.kp_joint[k];
        if (d.kp_joint[k] || d.kind == ILQR_SYS_JOINT || d.kind == ILQR_SYS_JOINT_TIME) {  // n_x x n_x precision: padded rows and columns 0
            for (int a = 0; a < mx.n_dev; a++)
                for (int b = 0; b < mx.n_dev; b++)
                    h.kp_Q[k][a * mx.n_dev + b] = (mx.usr[a] < 0 || mx.usr[b] < 0) ? 0.0 : d.kp_Q[k][mx.usr[a] * mx.n_user + mx.usr[b]];
        } else {  // PosOrn residual space: n_Q does not depend on dof
            for (int i = 0; i < dm.n_Q * dm.n_Q; i++) h.kp_Q[k][i] = d.kp_Q[k][i];
        }
        h.kp_dist[k] = d.kp_dist[k];
        h.kp_frame[k] = d.kp_has_frame[k];
        for (int i = 0; i < 9; i++) h.kp_fR[k][i] = d.kp_frame_R[k][i];
        for (int i = 0; i < 3; i++) h.kp_fp[k][i] = d.kp_frame_p[k][i];
        h.kp_has_Ru[k] = d.kp_has_Ru[k];
        for (int j = 0; j < mu.n_dev; j++) h.kp_Ru[k][j] = us(d.kp_Ru[k], j);
        h.kp_pos_radius[k] = d.kp_pos_radius[k];
        for (int i = 0; i < 3; i++) h.kp_orn_thresh[k][i] = d.kp_orn_thresh[k][i];
    }
    if (!build_step_table(h.kp_t, h.n_kp, h.steps)) return fail(c, "keypoint timesteps must be non-decreasing");
    h.reg = d.reg; h.alpha_floor = d.alpha_floor; h.stop_tol = d.stop_tol;
    return 0;
}

template <class T>
static int dalloc(ilqr_problem* p, T** ptr, size_t n, bool zero = true) {
    void* q = nullptr;
    if (n == 0) n = 1;
    HIPCHK(p->ctx, hipMalloc(&q, n * sizeof(T)));
    p->allocs.push_back(q);
    if (zero) HIPCHK(p->ctx, hipMemsetAsync(q, 0, n * sizeof(T), p->ctx->stream));
    *ptr = (T*)q;
    return 0;
}

extern "C" int ilqr_problem_create(ilqr_ctx* c, const ilqr_problem_desc* d, int batch, ilqr_problem** out) {
    if (!c) return 1;
    if (!d || !out || batch <= 0) return fail(c, "bad arguments");
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    auto* p = new ilqr_problem();
    p->ctx = c;
    p->desc = *d;
    p->B = batch;
    p->Bp = (batch + 63) / 64 * 64;
    // Row stride of every [row][Bp] buffer is Bp*8 bytes.  A power-of-two stride (Bp = 4096 -> 32 KiB) maps the 49 rows
    // of a K block onto the same L2 sets / HBM channel; one extra 64-instance pad column breaks the alignment.
    if (p->Bp % 512 == 0) p->Bp += 64;
    p->T = d->horizon;
    if (ilqr_dims_of(d, &p->udims)) { delete p; return fail(c, "unsupported system kind / nb_deriv"); }
    if (check_dof(c, d->dof) || !dof_map(d->kind, d->nb_deriv, d->dof, p->map)) { delete p; return 1; }
    {   // the device's dimensions: those of the same problem with 7 joints
        ilqr_problem_desc d7 = *d;
        d7.dof = DOF;
        (void)ilqr_dims_of(&d7, &p->dims);
    }
    p->mapped = !p->map.identity();
    p->qmap.n_user = d->dof; p->qmap.n_dev = DOF;
    for (int i = 0; i < MAP_MAX; i++) p->qmap.dev[i] = i < d->dof ? i : -1;
    index_map_fill_usr(p->qmap);
    if (lower_desc(c, *d, p->map, p->B, p->Bp, p->hdesc)) { delete p; return 1; }
    const int T = p->T, NX = p->dims.n_x, NU = p->dims.n_u, NF = p->dims.n_f, Bp = p->Bp;
    std::memset(&p->bufs, 0, sizeof(p->bufs));
    Bufs& b = p->bufs;
    int rc = 0;
    rc |= dalloc(p, &p->ddesc, 1);
    double *q0, *dq0, *U0, *tg;
    // the two buffers of X (of U) are the halves of ONE allocation, U padded to T rows: for n_x = n_u the two pairs have the same stride,
    // which lets the register-resident sweep address all four with one 32-bit offset per buffer (ilqr_kernels_dpp.hip)
    rc |= dalloc(p, &b.X[0], (size_t)2 * T * NX * Bp); b.X[1] = b.X[0] + (size_t)T * NX * Bp;
    rc |= dalloc(p, &b.U[0], (size_t)2 * T * NU * Bp); b.U[1] = b.U[0] + (size_t)T * NU * Bp;
    rc |= dalloc(p, &U0, (size_t)(T - 1) * NU * Bp);
    rc |= dalloc(p, &b.KD, (size_t)(T - 1) * Bp * NU * kd_rowp(NX));
    rc |= dalloc(p, &q0, (size_t)DOF * Bp);
    rc |= dalloc(p, &dq0, (size_t)DOF * Bp);
    rc |= dalloc(p, &tg, (size_t)(d->n_kp > 0 ? d->n_kp : 1) * NF * Bp);
    rc |= dalloc(p, &b.cost, Bp);
    rc |= dalloc(p, &b.alpha, Bp);
    rc |= dalloc(p, &b.cur, Bp);
    rc |= dalloc(p, &b.active, Bp);
    rc |= dalloc(p, &b.iters, Bp);
    rc |= dalloc(p, &b.status, Bp);
    rc |= dalloc(p, &b.pend, Bp);
    rc |= dalloc(p, &b.pred, Bp);
    rc |= dalloc(p, &b.lsc, (size_t)16 * Bp);
    rc |= dalloc(p, &b.dun, Bp);
    rc |= dalloc(p, &b.kpdev, (size_t)(d->n_kp > 0 ? d->n_kp : 1) * (NX + NU) * Bp);
    rc |= dalloc(p, &b.kpx, (size_t)(d->n_kp > 0 ? d->n_kp : 1) * 16 * (NX + NU) * Bp);
    rc |= dalloc(p, &b.dunA, (size_t)16 * Bp);
    {   // one slot per keypoint step; with shared steps the keypoints' own terms follow in a slot each (k_kp_terms, k_kp_sum)
        const int slots = p->hdesc.steps.n + (has_shared_step(p->hdesc.steps) ? d->n_kp : 0);
        rc |= dalloc(p, &b.kpd, (size_t)(slots > 0 ? slots : 1) * (NX + NX * NX) * Bp);
    }
    if (rc) { ilqr_problem_destroy(p); return 1; }
    b.U0 = U0; b.q0 = q0; b.dq0 = dq0; b.kp_tg = tg; b.desc = p->ddesc;
    bool up_ok = hipMemcpyAsync(p->ddesc, &p->hdesc, sizeof(DevDesc), hipMemcpyHostToDevice, c->stream) == hipSuccess;
    if (p->B >= SPLIT_MIN_BATCH) {  // halves for the two-stream solve
        p->half_b0[0] = 0;
        p->half_B[0] = split_first_half(p->B);
        p->half_b0[1] = p->half_B[0];
        p->half_B[1] = p->B - p->half_B[0];
        for (int i = 0; i < 2 && up_ok; i++) {
            DevDesc hd = p->hdesc;
            hd.B = p->half_B[i];
            up_ok = dalloc(p, &p->ddesc_half[i], 1) == 0 &&
                    hipMemcpyAsync(p->ddesc_half[i], &hd, sizeof(DevDesc), hipMemcpyHostToDevice, c->stream) == hipSuccess &&
                    hipStreamSynchronize(c->stream) == hipSuccess;  // hd is a stack copy
        }
    }
    if (!up_ok || hipStreamSynchronize(c->stream) != hipSuccess) {
        ilqr_problem_destroy(p);
        return fail(c, "descriptor upload failed");
    }
    c->problems.push_back(p);
    *out = p;
    return 0;
}

extern "C" void ilqr_problem_destroy(ilqr_problem* p) {
    if (!p) return;
    for (auto it = p->ctx->problems.begin(); it != p->ctx->problems.end(); ++it)
        if (*it == p) { p->ctx->problems.erase(it); break; }
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    for (void* q : p->allocs) (void)hipFree(q);
    for (const void* q : {(const void*)p->obs.geom, (const void*)p->obs.obs, (const void*)p->obs.obd, (const void*)p->obs_dense.sd, (const void*)p->obs_dense.part}) (void)hipFree((void*)q);
    for (DevScratch* b : {&p->staging, &p->cl_kpx, &p->cl_rep, &p->cl_con_ws, &p->cl_cost, &p->cl_cov_ws, &p->cl_cov_kps, &p->ms_idx, &p->ms_out}) b->release();
    batchcp_free(p->cp);
    batchwide_free(p->cpw);
    delete p;
}

// natural [B][rows] host or device array -> SoA [rows][Bp] device buffer; with a map m: natural [B][outer][m->n_user] -> [outer][m->n_dev][Bp]
// (rows = outer * m->n_user), the padding written as 0
static int upload(ilqr_problem* p, const double* src, bool src_is_dev, double* dst, int rows, const IndexMap* m = nullptr, int outer = 0) {
    ilqr_ctx* c = p->ctx;
    const size_t n = (size_t)p->B * rows;
    const double* dsrc = src;
    if (!src_is_dev) {
        if (p->staging.reserve(c, n)) return 1;
        HIPCHK(c, hipMemcpyAsync(p->staging.ptr, src, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        dsrc = p->staging.ptr;
    }
    if (m) launch_to_soa_map(dsrc, dst, p->B, p->Bp, outer, *m, c->stream);
    else launch_to_soa(dsrc, dst, p->B, p->Bp, rows, c->stream);
    HIPCHK(c, hipGetLastError());
    if (!src_is_dev) HIPCHK(c, hipStreamSynchronize(c->stream));  // staging is reused; the host buffer may go away
    return 0;
}

static int set_init_state(ilqr_problem* p, const double* q0, const double* dq0, bool dev) {
    if (!p) return 1;
    if (!q0) return fail(p->ctx, "q0 is required");
    p->has_gains = p->has_plan = false;
    const IndexMap* qm = p->mapped ? &p->qmap : nullptr;
    if (upload(p, q0, dev, (double*)p->bufs.q0, p->desc.dof, qm, 1)) return 1;
    if (dq0) {
        if (upload(p, dq0, dev, (double*)p->bufs.dq0, p->desc.dof, qm, 1)) return 1;
    } else {
        HIPCHK(p->ctx, hipMemsetAsync((void*)p->bufs.dq0, 0, sizeof(double) * DOF * p->Bp, p->ctx->stream));
    }
    p->has_state = true;
    return 0;
}
extern "C" int ilqr_problem_set_init_state(ilqr_problem* p, const double* q0, const double* dq0) { return set_init_state(p, q0, dq0, false); }
extern "C" int ilqr_problem_set_init_state_dev(ilqr_problem* p, const double* q0, const double* dq0) { return set_init_state(p, q0, dq0, true); }

static int set_kp(ilqr_problem* p, int k, const double* tg, bool dev) {
    if (!p) return 1;
    if (k < 0 || k >= p->desc.n_kp || !tg) return fail(p->ctx, "bad keypoint index / null target");
    p->has_gains = p->has_plan = false;
    double* dst = (double*)p->bufs.kp_tg + (size_t)k * p->dims.n_f * p->Bp;
    if (p->mapped && (p->desc.kind == ILQR_SYS_JOINT || p->desc.kind == ILQR_SYS_JOINT_TIME))  // the target is a state
        return upload(p, tg, dev, dst, p->udims.n_f, &p->map.x, 1);
    if (p->mapped && p->desc.kp_joint[k]) {  // joint vector (+ time) in the first n_x of the n_f slots
        const IndexMap tm = joint_target_map(p->map, p->dims.n_f);
        return upload(p, tg, dev, dst, p->udims.n_f, &tm, 1);
    }
    return upload(p, tg, dev, dst, p->udims.n_f);
}
extern "C" int ilqr_problem_set_keypoint_targets(ilqr_problem* p, int k, const double* tg) { return set_kp(p, k, tg, false); }
extern "C" int ilqr_problem_set_keypoint_targets_dev(ilqr_problem* p, int k, const double* tg) { return set_kp(p, k, tg, true); }

static int set_controls(ilqr_problem* p, const double* U0, bool dev) {
    if (!p) return 1;
    if (!U0) return fail(p->ctx, "U0 is required");
    p->has_gains = p->has_plan = false;
    if (upload(p, U0, dev, (double*)p->bufs.U0, (p->T - 1) * p->udims.n_u, p->mapped ? &p->map.u : nullptr, p->T - 1)) return 1;
    p->has_controls = true;
    p->u0_zero = false;
    if (!dev) {
        const size_t n = (size_t)p->B * (p->T - 1) * p->udims.n_u;
        size_t i = 0;
        while (i < n && U0[i] == 0.0) i++;
        p->u0_zero = (i == n);
    }
    return 0;
}
extern "C" int ilqr_problem_set_controls(ilqr_problem* p, const double* U0) { return set_controls(p, U0, false); }
extern "C" int ilqr_problem_set_controls_dev(ilqr_problem* p, const double* U0) { return set_controls(p, U0, true); }

extern "C" int ilqr_problem_set_constraints(ilqr_problem* p, int m, int per_step, const double* A, const double* b, const double* lambda0) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    if (m <= 0 || !A || !b) return fail(c, "bad constraint arguments");
    p->has_gains = p->has_plan = false;
    const int ns = p->dims.n_x + p->dims.n_u, T = p->T, nsu = p->udims.n_x + p->udims.n_u;
    const size_t nk = per_step ? (size_t)(T - 1) : 1;
    if (p->bufs.m != m || p->bufs.per_step != per_step || !p->conA) {
        if (p->conA) {  // another shape: release the previous constraint buffers (nothing in flight may still read them)
            HIPCHK(c, hipStreamSynchronize(c->stream));
            void* old[5] = {p->conA, p->conb, p->bufs.lambda, p->bufs.Is, p->lambda0};
            for (void* q : old) {
                for (auto it = p->allocs.begin(); it != p->allocs.end(); ++it)
                    if (*it == q) { p->allocs.erase(it); break; }
                (void)hipFree(q);
            }
            p->conA = p->conb = p->lambda0 = nullptr;
            p->bufs.lambda = p->bufs.Is = nullptr;
            p->bufs.m = 0;
        }
        if (dalloc(p, &p->conA, nk * m * ns) || dalloc(p, &p->conb, nk * m)) return 1;
        double *lam, *Is;
        if (dalloc(p, &lam, (size_t)(T - 1) * m * p->Bp) || dalloc(p, &Is, (size_t)(T - 1) * m * p->Bp)) return 1;
        p->bufs.lambda = lam;
        p->bufs.Is = Is;
        if (dalloc(p, &p->lambda0, (size_t)(T - 1) * m * p->Bp)) return 1;
    }
    std::vector<double> Aw;  // columns of the [x; u] layout through the map: padded columns 0
    if (p->mapped) {
        const IndexMap &mx = p->map.x, &mu = p->map.u;
        Aw.assign(nk * m * ns, 0.0);
        for (size_t r = 0; r < nk * m; r++) {
            for (int j = 0; j < mx.n_user; j++) Aw[r * ns + mx.dev[j]] = A[r * nsu + j];
            for (int i = 0; i < mu.n_user; i++) Aw[r * ns + mx.n_dev + mu.dev[i]] = A[r * nsu + mx.n_user + i];
        }
    }
    HIPCHK(c, hipMemcpyAsync(p->conA, p->mapped ? Aw.data() : A, nk * m * ns * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p->conb, b, nk * m * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    p->bufs.m = m; p->bufs.per_step = per_step; p->bufs.conA = p->conA; p->bufs.conb = p->conb;
    p->con_state_only = true;
    for (size_t k = 0; k < nk * m; k++)
        for (int j = p->udims.n_x; j < nsu; j++)
            if (A[k * nsu + j] != 0.0) p->con_state_only = false;
    if (lambda0) {
        if (upload(p, lambda0, false, p->bufs.lambda, (T - 1) * m)) return 1;
    } else {
        HIPCHK(c, hipMemsetAsync(p->bufs.lambda, 0, sizeof(double) * (size_t)(T - 1) * m * p->Bp, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(p->lambda0, p->bufs.lambda, sizeof(double) * (size_t)(T - 1) * m * p->Bp, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

extern "C" int ilqr_problem_reset_multipliers(ilqr_problem* p) {
    if (!p) return 1;
    if (p->bufs.m <= 0) return fail(p->ctx, "no constraints set");
    p->has_gains = p->has_plan = false;
    HIPCHK(p->ctx, hipMemcpyAsync(p->bufs.lambda, p->lambda0, sizeof(double) * (size_t)(p->T - 1) * p->bufs.m * p->Bp,
                                  hipMemcpyDeviceToDevice, p->ctx->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------ solvers

static int ensure_trace(ilqr_problem* p, int nb_iter) {
    if (nb_iter > p->trace_iters) {
        double *ct, *at;
        if (dalloc(p, &ct, (size_t)nb_iter * p->Bp, false) || dalloc(p, &at, (size_t)nb_iter * p->Bp, false)) return 1;
        p->bufs.cost_trace = ct;
        p->bufs.alpha_trace = at;
        p->trace_iters = nb_iter;
    }
    if (nb_iter > 0) {  // NaN-fill: entries after an instance's early stop stay NaN
        HIPCHK(p->ctx, hipMemsetAsync(p->bufs.cost_trace, 0xFF, sizeof(double) * (size_t)nb_iter * p->Bp, p->ctx->stream));
        HIPCHK(p->ctx, hipMemsetAsync(p->bufs.alpha_trace, 0xFF, sizeof(double) * (size_t)nb_iter * p->Bp, p->ctx->stream));
    }
    return 0;
}

// The buffer table of one half of a split problem: every per-instance array is [..][Bp] with the instance innermost, so a half is the
// same table with the base pointers moved by its first instance (gain records: by whole records) and its own descriptor (B = its size).
static Bufs half_bufs(const ilqr_problem* p, int half) {
    Bufs v = p->bufs;
    const size_t o = (size_t)p->half_b0[half];
    v.desc = p->ddesc_half[half];
    for (int i = 0; i < 2; i++) { v.X[i] += o; v.U[i] += o; }
    v.U0 += o; v.q0 += o; v.dq0 += o; v.kp_tg += o;
    v.KD += o * (size_t)kd_rs(p->bufs.kd_sym, p->dims.n_u, kd_rowp(p->dims.n_x));
    v.cost += o; v.alpha += o; v.cur += o; v.active += o; v.iters += o; v.status += o; v.kpd += o; v.pend += o; v.pred += o;
    v.lsc += o; v.dun += o; v.kpdev += o; v.kpx += o; v.dunA += o;
    if (v.ws) v.ws += o;
    if (v.cost_trace) { v.cost_trace += o; v.alpha_trace += o; }
    if (v.lambda) { v.lambda += o; v.Is += o; }
    return v;
}

// Which kernels run is decided by plan_riccati (ilqr_plan.hpp) from the problem's shape, the batch size and the context's pins: by default the
// cooperative kernels, all step sizes of the line search in one pass; ilqr_ctx_set_crosscheck(ctx, 1, ..) forces the generic lane-per-instance
// kernels, the cross-check set of the parity tests.  The library reads NO environment variable: the pins are context state.
static PlanIn plan_input(const ilqr_problem* p, bool al, int nb_iter, int line_search) {
    const ilqr_ctx* c = p->ctx;
    const int T = p->T;
    PlanIn in;
    in.kind = p->desc.kind; in.nd = p->desc.nb_deriv; in.al = al; in.m = p->bufs.m; in.per_step = p->bufs.per_step; in.con_state_only = p->con_state_only;
    in.limits2_set = p->desc.limits2_set != 0;
    in.shared_steps = has_shared_step(p->hdesc.steps);
    in.obstacles = p->has_obs;
    in.obstacles_coop = c->obs_coop;
    in.uniform_R = true;
    for (int i = 1; i < p->dims.n_u; i++) in.uniform_R = in.uniform_R && (p->hdesc.R_diag[i] == p->hdesc.R_diag[0]);
    // the register-resident sweep addresses x, u and the multipliers with 32-bit byte offsets (ilqr_kernels_dpp.hip): batches whose arrays pass
    // 4 GiB (T * Bp beyond ~38 M) take the other sweeps
    in.off32 = (size_t)2 * T * p->dims.n_x * p->Bp * 8 < ((size_t)1 << 32) && (size_t)T * (p->bufs.m > 0 ? p->bufs.m : 1) * p->Bp * 8 < ((size_t)1 << 32);
    in.line_search = line_search != 0; in.alpha_floor = p->desc.alpha_floor; in.nb_iter = nb_iter;
    in.B = p->B; in.n_simd = c->n_simd; in.halves = p->ddesc_half[0] != nullptr; in.split = c->split; in.profile = c->profile;
    in.generic = c->xc_generic; in.sweep = c->xc_sweep; in.forward = c->xc_forward; in.reroll = c->xc_reroll;
    return in;
}

// ---- one or two independent halves ("lanes" of the launch schedule).  Instances never interact, so the halves of a large batch are
// two complete solves on two streams; the second one starts one sweep later, so that its latency-bound sweep runs under the other
// half's bandwidth-bound forward pass.  Results do not depend on the split (bit for bit: tests/test_gpu_fullsize.py).
struct Half { Bufs bufs; int B; hipStream_t st; };
static int split_begin(ilqr_problem* p, bool split, Half hv[2], int& nh) {
    ilqr_ctx* c = p->ctx;
    nh = 1;
    if (!split) {
        hv[0].bufs = p->bufs; hv[0].B = p->B; hv[0].st = c->stream;
        return 0;
    }
    for (int i = 0; i < 2; i++) {
        if (!c->half_stream[i]) HIPCHK(c, hipStreamCreateWithFlags(&c->half_stream[i], hipStreamNonBlocking));
        if (!c->ev_half_done[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_half_done[i], hipEventDisableTiming));
    }
    if (!c->ev_begin) HIPCHK(c, hipEventCreateWithFlags(&c->ev_begin, hipEventDisableTiming));
    if (!c->ev_stagger) HIPCHK(c, hipEventCreateWithFlags(&c->ev_stagger, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev_begin, c->stream));  // inputs (and the trace fill) are ordered on the caller's stream
    nh = 2;
    for (int i = 0; i < 2; i++) {
        HIPCHK(c, hipStreamWaitEvent(c->half_stream[i], c->ev_begin, 0));
        hv[i].bufs = half_bufs(p, i); hv[i].B = p->half_B[i]; hv[i].st = c->half_stream[i];
    }
    return 0;
}
// Join on EVERY exit path: an early return between split_begin and the end of the call (a failed launch or event call on one half) must not
// leave work queued on a half stream that the context's stream never waits for -- the caller's next call would race with it.
struct SplitJoin {
    ilqr_ctx* c; bool on;
    ~SplitJoin() {
        if (!on) return;
        for (int i = 0; i < 2; i++)
            if (hipEventRecord(c->ev_half_done[i], c->half_stream[i]) != hipSuccess || hipStreamWaitEvent(c->stream, c->ev_half_done[i], 0) != hipSuccess)
                (void)hipStreamSynchronize(c->half_stream[i]);  // last resort: drain it here
    }
};

// What k_kp_derivs needs of a launch (and what every FwdArgs of a plan shares): the step table's sizes and which keypoint code is instantiated.
static FwdArgs plan_fwd_args(const ilqr_problem* p, const RiccatiPlan& pl) {
    FwdArgs f;
    std::memset(&f, 0, sizeof(f));
    f.n_alpha = pl.n_alpha; f.n_kp = p->hdesc.steps.n;
    f.shared = has_shared_step(p->hdesc.steps) ? 1 : 0;
    f.n_kp_all = p->desc.n_kp;
    f.fused = pl.fused ? 1 : 0;
    f.fwd_lds = pl.fwd_lds ? 1 : 0;
    f.fwd_io = pl.fwd_io ? 1 : 0;
    f.limits = p->desc.limits_set ? 1 : 0;
    for (int k = 0; k < p->desc.n_kp; k++) f.kp_ext |= p->desc.kp_dist[k] | p->desc.kp_has_frame[k] | p->desc.kp_has_Ru[k] | p->desc.kp_joint[k];
    return f;
}
// The sweep of the plan on half h (the whole batch: h = 0)
static void launch_sweep(const ilqr_problem* p, const RiccatiPlan& pl, int h, bool al, const Bufs& bf, int B, hipStream_t st, SweepArgs& sw) {
    const int kind = p->desc.kind, nd = p->desc.nb_deriv;
    switch (pl.sweep) {
        case Sweep::SiDpp: sw.si_wg = pl.si_wg[h] ? 1 : 0; sw.si_io = pl.si_io[h] ? 1 : 0; sw.si_prep = pl.si_prep[h] ? 1 : 0; launch_backward_si_dpp(al, pl.fused, pl.kd_sym == 1, pl.si_lanes[h], bf, B, st, sw); break;
        case Sweep::Rows: launch_backward_rows(kind, nd, al, bf, B, st); break;
        case Sweep::Mfma: launch_backward_mfma(kind, nd, al, bf, B, st); break;
        case Sweep::Generic: launch_backward_generic(kind, nd, al, bf, B, st, p->has_obs ? &p->obs : nullptr); break;
    }
}
// l_x, l_xx of the obstacle terms at every step of the current trajectory, where k_kp_derivs runs: before every sweep.  (A problem with these
// terms is never split: plan_riccati keeps it on the generic kernels or on its unsplit cooperative path.)  On the cooperative path
// (RiccatiPlan::obs_dense) k_stage_dense then forms l_x | l_xx of every stage for k_backward_si_dpp<.., SW_DENSE>, behind k_kp_derivs.
static void launch_obs_terms(const ilqr_problem* p, const RiccatiPlan& pl, const Bufs& bf, int B, hipStream_t st) {
    if (!p->has_obs) return;
    if (p->obs.n_anchor) launch_obs_derivs_self(bf, p->obs, B, p->T, p->dims.n_x, 0, st);   // a geometry with self pairs
    else launch_obs_derivs(bf, p->obs, B, p->T, p->dims.n_x, 0, st);
    if (pl.obs_dense) launch_stage_dense(bf, p->obs, p->obs_dense.sd, B, p->T, 0, st);
}
// The buffers of the cooperative path, at its first use; freed with the problem
static int ensure_obs_dense(ilqr_problem* p) {
    ilqr_ctx* c = p->ctx;
    const int N = p->dims.n_x;
    if (!p->obs_dense.sd) HIPCHK(c, hipMalloc((void**)&p->obs_dense.sd, sizeof(double) * (size_t)p->T * (size_t)(N + N * N) * (size_t)p->Bp));
    if (!p->obs_dense.part) HIPCHK(c, hipMalloc((void**)&p->obs_dense.part, sizeof(double) * (size_t)p->T * OBS_LS_ROWS * (size_t)p->Bp));
    return 0;
}

static int solve_riccati(ilqr_problem* p, bool al, int nb_iter, int lag, double penalty0, double scaling, int line_search, int early_stop) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    if (!p->has_state || !p->has_controls) return fail(c, "set_init_state and set_controls must be called before a solve");
    if (nb_iter < 0) return fail(c, "nb_iter < 0");
    if (al && (p->bufs.m <= 0 || lag <= 0)) return fail(c, "AL solve needs constraints (ilqr_problem_set_constraints) and lag_update_step > 0");
    HIPCHK(c, hipSetDevice(c->device));
    if (ensure_trace(p, nb_iter)) return 1;
    p->last_nb_iter = nb_iter;
    p->has_gains = p->has_plan = false;  // until this solve's launches are queued; a 0-iteration solve re-rolls X from U0 and leaves the gains of another plan
    const int kind = p->desc.kind, nd = p->desc.nb_deriv, T = p->T;
    const RiccatiPlan pl = plan_riccati(plan_input(p, al, nb_iter, line_search));
    if (pl.kd_sym != KD_SYM_KEEP) p->bufs.kd_sym = pl.kd_sym;  // before half_bufs: it sizes the half's offset into KD
    if (pl.needs_ws && !p->bufs.ws)
        if (dalloc(p, &p->bufs.ws, (size_t)backward_ws_entries(kind, nd) * p->Bp, false)) return 1;
    if (pl.obs_dense && ensure_obs_dense(p)) return 1;

    Half hv[2];
    int nh = 1;
    if (split_begin(p, pl.split, hv, nh)) return 1;
    SplitJoin split_join{c, pl.split};  // on every exit path
    FwdArgs f = plan_fwd_args(p, pl);
    f.line_search = line_search; f.early_stop = early_stop; f.nb_iter = nb_iter; f.penalty_roll = penalty0; f.al = al ? 1 : 0;
    if (pl.obs_dense) { f.obs = &p->obs; f.obs_part = p->obs_dense.part; f.obs_T = T; }  // launch_forward_wave: the obstacle cost of every step size
    for (int h = 0; h < nh; h++) {
        const Bufs& bf = hv[h].bufs;
        ProfScope ps(c, ILQR_PROF_ROLLOUT);
        if (pl.init == Init::Lti) launch_init_lti(kind, nd, bf, hv[h].B, hv[h].st);
        else if (p->has_obs && p->obs.n_anchor) launch_init_self(kind, nd, al, bf, hv[h].B, hv[h].st, penalty0, p->obs);   // a geometry with self pairs
        else launch_init(kind, nd, al, bf, hv[h].B, hv[h].st, penalty0, p->has_obs ? &p->obs : nullptr);
        if (pl.obs_dense) launch_obs_ls(bf, p->obs, p->obs_dense.part, hv[h].B, T, p->dims.n_x, 1, 1, hv[h].st);  // the initial trajectory's obstacle cost joins cost, behind k_init_finish
        if (pl.init_al_update) {  // active-set weights of the initial trajectory: I_k = penalty * (g<0 && lambda==0 ? 0 : 1)
            f.it = -1; f.do_update = 0;
            launch_al_update(kind, nd, bf, hv[h].B, T, hv[h].st, f);
        }
    }
    HIPCHK(c, hipGetLastError());
    double penalty = penalty0;
    SweepArgs sw;
    sw.pen_in = penalty; sw.pen_update_prev = penalty; sw.do_update_prev = 0; sw.si_wg = 0; sw.si_io = 0; sw.si_prep = 0;
    sw.sd = pl.obs_dense ? p->obs_dense.sd : nullptr;
    for (int it = 0; it < nb_iter; it++) {
        FwdArgs fi = f;
        fi.it = it;
        fi.penalty_roll = penalty;  // I_k is stored pre-multiplied by the penalty current at rollout time (AL-ILQR.cpp:190)
        fi.do_update = al && ((it + 1) % lag == 0);
        if (fi.do_update) penalty *= scaling;  // multipliers use the UPDATED penalty (AL-ILQR.cpp:203-205)
        fi.penalty_update = penalty;
        for (int h = 0; h < nh; h++) {
            const Bufs& bf = hv[h].bufs;
            const int B = hv[h].B;
            hipStream_t st = hv[h].st;
            if (pl.split && it == 0 && h == 1) HIPCHK(c, hipStreamWaitEvent(st, c->ev_stagger, 0));  // one sweep behind the first half
            {   // l_x, l_xx at the keypoint steps (FK, log map, J'QJ) for every sweep: none of them holds keypoint code
                ProfScope ps(c, ILQR_PROF_OTHER);
                launch_kp_derivs(kind, nd, bf, B, st, fi);
                launch_obs_terms(p, pl, bf, B, st);
            }
            {
                ProfScope ps(c, ILQR_PROF_BACKWARD);
                launch_sweep(p, pl, h, al, bf, B, st, sw);
            }
            if (pl.split && it == 0 && h == 0) HIPCHK(c, hipEventRecord(c->ev_stagger, st));
            {
                ProfScope ps(c, ILQR_PROF_FORWARD);
                switch (pl.forward) {
                    case Forward::WaveWg: launch_forward_wave(kind, false, bf, B, st, fi); break;
                    case Forward::WaveDpp: launch_forward_wave(kind, true, bf, B, st, fi); break;
                    case Forward::Lin: launch_forward_lin(bf, B, st, fi); break;
                    case Forward::Mfma: launch_forward_tm(kind, nd, bf, B, st, fi); break;
                    case Forward::Generic:
                        if (p->has_obs && p->obs.n_anchor) launch_forward_generic_self(kind, nd, al, bf, B, st, fi, p->obs);   // a geometry with self pairs
                        else launch_forward_generic(kind, nd, al, bf, B, st, fi, p->has_obs ? &p->obs : nullptr);
                        break;
                }
            }
            if (pl.apply != Apply::None && (pl.apply != Apply::WaveLast || it == nb_iter - 1)) {
                ProfScope ps(c, ILQR_PROF_APPLY);
                switch (pl.apply) {
                    case Apply::Wave: case Apply::WaveLast: launch_apply_wave(kind, bf, B, T, st, fi); break;
                    case Apply::Lin: launch_apply_lin(bf, B, T, st); break;
                    case Apply::RerollRows: case Apply::RerollDpp: launch_apply_tm(kind, nd, pl.apply == Apply::RerollDpp, bf, B, st, fi); break;
                    case Apply::None: break;
                }
            }
            if (pl.al_update) {  // active-set weights of the accepted trajectory (+ multiplier update every `lag` iterations)
                ProfScope ps(c, ILQR_PROF_OTHER);
                launch_al_update(kind, nd, bf, B, T, st, fi);
            }
        }
        sw.pen_in = fi.penalty_roll; sw.pen_update_prev = fi.penalty_update; sw.do_update_prev = fi.do_update;  // for the next sweep
        HIPCHK(c, hipGetLastError());
    }
    // (the caller's stream continues when both halves are done: SplitJoin above, on every exit path)
    prof_mark(c, -1);
    p->has_gains = nb_iter >= 1;
    p->has_plan = true;
    return 0;
}

extern "C" int ilqr_solve_recursive(ilqr_problem* p, int nb_iter, int line_search, int early_stop) {
    return solve_riccati(p, false, nb_iter, 1, 0.0, 1.0, line_search, early_stop);
}
extern "C" int ilqr_solve_al(ilqr_problem* p, int nb_iter, int lag, double penalty, double scaling, int line_search, int early_stop) {
    return solve_riccati(p, true, nb_iter, lag, penalty, scaling, line_search, early_stop);
}

// The batch solvers' sparse form stacks one target block per keypoint of the reference's concatenated list, and at a shared timestep the
// reference's SequentialSystem stacks every sub-system's target into each of them (getMuVector(true) / getQMatrix(true)): not reproduced.
static const char* const BATCH_SHARED_STEP_TEXT =
    "keypoints that share a timestep are not supported by the batch solvers (ilqr_solve_batch_cp, ilqr_solve_batch)";
// The batch solvers' normal equations hold the keypoint and limit terms only.
static const char* const BATCH_OBSTACLES_TEXT =
    "obstacle terms are not supported by the batch solvers (ilqr_solve_batch_cp, ilqr_solve_batch): remove them (ilqr_problem_set_obstacles with robot = NULL) or use ilqr_solve_recursive / ilqr_solve_al";

extern "C" int ilqr_solve_batch_cp(ilqr_problem* p, const double* psi, int Kw, int nb_iter, int early_stop) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    if (has_shared_step(p->hdesc.steps)) return fail(c, BATCH_SHARED_STEP_TEXT);
    if (p->has_obs) return fail(c, BATCH_OBSTACLES_TEXT);
    if (!p->has_state || !p->has_controls) return fail(c, "set_init_state and set_controls must be called before a solve");
    p->has_gains = p->has_plan = false;  // the batch solvers leave no gains (ilqr_problem_gains computes them about the plan)
    HIPCHK(c, hipSetDevice(c->device));
    std::string err;
    if (ensure_trace(p, nb_iter)) return 1;
    p->last_nb_iter = nb_iter;
    const bool cp_time = p->desc.kind == ILQR_SYS_POS_ORN_TIME || p->desc.kind == ILQR_SYS_JOINT_TIME;
    std::vector<double> psiw;  // PSI on the device's controls: zero rows for the padded ones (they never move)
    if (psi && Kw > 0 && p->mapped) {
        const IndexMap& mu = p->map.u;
        psiw.assign((size_t)(p->T - 1) * mu.n_dev * Kw, 0.0);
        for (int k = 0; k < p->T - 1; k++)
            for (int i = 0; i < mu.n_user; i++)
                std::memcpy(&psiw[((size_t)k * mu.n_dev + mu.dev[i]) * Kw], psi + ((size_t)k * mu.n_user + i) * Kw, sizeof(double) * Kw);
        psi = psiw.data();
    }
    if (psi && Kw > 16 && !(cp_time && Kw <= 32)) {  // wide basis: low-rank form of the normal equations (ilqr_batchwide.hip)
        if (batchwide_solve(p->cpw, p->hdesc, p->bufs, p->dims.n_x, p->dims.n_u, psi, Kw, nb_iter, early_stop, p->u0_zero, c->stream, err, prof_hook(c))) return fail(c, err);
        prof_mark(c, -1);
        p->has_plan = true;
        return 0;
    }
    p->cp.xc_lane_solve = c->xc_cp_lane; p->cp.xc_general = c->xc_cp_general;
    if (batchcp_solve(p->cp, p->hdesc, p->bufs, p->dims.n_x, p->dims.n_u, p->dims.n_f, p->dims.n_Q, psi, Kw, nb_iter, early_stop, c->stream, err, prof_hook(c)))
        return fail(c, err);
    prof_mark(c, -1);
    p->has_plan = true;
    return 0;
}

extern "C" int ilqr_solve_batch(ilqr_problem* p, int nb_iter, int early_stop) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    if (has_shared_step(p->hdesc.steps)) return fail(c, BATCH_SHARED_STEP_TEXT);
    if (p->has_obs) return fail(c, BATCH_OBSTACLES_TEXT);
    if (!p->has_state || !p->has_controls) return fail(c, "set_init_state and set_controls must be called before a solve");
    p->has_gains = p->has_plan = false;  // the batch solvers leave no gains (ilqr_problem_gains computes them about the plan)
    HIPCHK(c, hipSetDevice(c->device));
    std::string err;
    if (ensure_trace(p, nb_iter)) return 1;
    p->last_nb_iter = nb_iter;
    if (batchwide_solve(p->cpw, p->hdesc, p->bufs, p->dims.n_x, p->dims.n_u, nullptr, 0, nb_iter, early_stop, p->u0_zero, c->stream, err, prof_hook(c))) return fail(c, err);
    prof_mark(c, -1);
    p->has_plan = true;
    return 0;
}

// One backward pass (ILQRRecursive.cpp:68-97) about the plan the problem holds, whichever solver left it: k_gains_prepare, k_kp_derivs and the
// sweep plan_riccati chooses for ilqr_solve_recursive(p, 1, 1, 0) -- no augmented-Lagrangian terms, no rollout, no line search.  Nothing is
// pending when it starts: the fused path applies the last winner itself (Apply::WaveLast on the last iteration, and an instance that stopped
// early before it is applied by the following sweep), every other path applies or flips inside the iteration that decided, and the batch
// solvers clear `pend` in their rollout and never set it.  So X[cur], U[cur] are the plan of every instance, active or not.
//
// With al (ilqr_problem_gains_al): the backward pass of AL-ILQR.cpp:94-145, i.e. the sweep chosen for ilqr_solve_al(p, 1, ..) with the active-set
// weights of the held plan and the multipliers as they are -- k_gains_al_weights forms Is for the sweeps that read it; the fused sweep forms its
// weights itself from SweepArgs::pen_in.  Is is scratch: every AL solve re-forms it before a sweep reads it (k_init_rollout<.., AL> on the generic
// path, k_al_post at it = -1 behind the LTI rollout, and the fused sweep never reads it), and nothing else reads it.
static int gains_about_plan(ilqr_problem* p, bool al, double penalty) {
    ilqr_ctx* c = p->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    const int kind = p->desc.kind, nd = p->desc.nb_deriv;
    const RiccatiPlan pl = plan_riccati(plan_input(p, al, 1, 1));
    p->has_gains = false;  // until the sweep is queued
    p->bufs.kd_sym = pl.kd_sym;  // before half_bufs: it sizes the half's offset into KD
    if (pl.needs_ws && !p->bufs.ws)
        if (dalloc(p, &p->bufs.ws, (size_t)backward_ws_entries(kind, nd) * p->Bp, false)) return 1;
    if (pl.obs_dense && ensure_obs_dense(p)) return 1;
    Half hv[2];
    int nh = 1;
    if (split_begin(p, pl.split, hv, nh)) return 1;
    SplitJoin split_join{c, pl.split};  // on every exit path
    const FwdArgs f = plan_fwd_args(p, pl);
    SweepArgs sw;
    sw.pen_in = penalty; sw.pen_update_prev = penalty; sw.do_update_prev = 0; sw.si_wg = 0; sw.si_io = 0; sw.si_prep = 0;
    sw.sd = pl.obs_dense ? p->obs_dense.sd : nullptr;
    for (int h = 0; h < nh; h++) {
        const Bufs& bf = hv[h].bufs;
        const int B = hv[h].B;
        hipStream_t st = hv[h].st;
        {
            ProfScope ps(c, ILQR_PROF_OTHER);
            launch_gains_prepare(bf, B, st);
        }
        if (al && !pl.fused) {  // the sweeps that read Is
            ProfScope ps(c, ILQR_PROF_OTHER);
            launch_gains_al_weights(kind, nd, bf, B, p->T, penalty, st);
        }
        {
            ProfScope ps(c, ILQR_PROF_OTHER);
            launch_kp_derivs(kind, nd, bf, B, st, f);
            launch_obs_terms(p, pl, bf, B, st);
        }
        {
            ProfScope ps(c, ILQR_PROF_BACKWARD);
            launch_sweep(p, pl, h, al, bf, B, st, sw);
        }
    }
    HIPCHK(c, hipGetLastError());
    prof_mark(c, -1);
    p->has_gains = true;
    return 0;
}

extern "C" int ilqr_problem_gains(ilqr_problem* p) {
    if (!p) return 1;
    if (!p->has_plan)
        return fail(p->ctx, "ilqr_problem_gains needs a plan: run a solver since the problem's inputs last changed (ilqr_solve_recursive with nb_iter = 0 rolls out the controls as they are)");
    return gains_about_plan(p, false, 0.0);
}

extern "C" int ilqr_problem_gains_al(ilqr_problem* p, double penalty) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    if (p->bufs.m <= 0)
        return fail(c, "ilqr_problem_gains_al needs constraint rows: call ilqr_problem_set_constraints, then a solver (ilqr_problem_gains sweeps without them)");
    if (!p->has_plan)
        return fail(c, "ilqr_problem_gains_al needs a plan: run a solver since the problem's inputs and constraints last changed (ilqr_solve_al with nb_iter = 0 rolls out the controls as they are)");
    if (!(std::isfinite(penalty) && penalty >= 0.0))
        return fail(c, "ilqr_problem_gains_al: the penalty must be finite and >= 0 (got " + std::to_string(penalty) + "): pass the penalty the plan's solve ended with, or its initial one");
    return gains_about_plan(p, true, penalty);
}

// ------------------------------------------------------------------------------------------------ results

enum { GET_PLAIN, GET_CUR, GET_SCALED };
// SoA [rows][Bp] -> natural [B][rows]; with a map m (GET_CUR only): [outer][m->n_dev][Bp] -> natural [B][outer][m->n_user], rows = outer * m->n_user
static int download(ilqr_problem* p, int mode, const double* s0, const double* s1, double* dst, bool dst_is_dev, int rows, const IndexMap* m = nullptr,
                    int outer = 0) {
    ilqr_ctx* c = p->ctx;
    if (!dst) return fail(c, "null output pointer");
    const size_t n = (size_t)p->B * rows;
    double* ddst = dst;
    if (!dst_is_dev) {
        if (p->staging.reserve(c, n)) return 1;
        ddst = p->staging.ptr;
    }
    if (m) launch_from_soa_cur_map(s0, s1, p->bufs.cur, ddst, p->B, p->Bp, outer, *m, c->stream);
    else if (mode == GET_CUR) launch_from_soa_cur(s0, s1, p->bufs.cur, ddst, p->B, p->Bp, rows, c->stream);
    else if (mode == GET_SCALED) launch_from_soa_scaled(s0, p->bufs.alpha, p->bufs.iters, ddst, p->B, p->Bp, rows, c->stream);
    else launch_from_soa(s0, ddst, p->B, p->Bp, rows, c->stream);
    HIPCHK(c, hipGetLastError());
    if (!dst_is_dev) {
        HIPCHK(c, hipMemcpyAsync(dst, p->staging.ptr, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

static int get_X(ilqr_problem* p, double* X, bool dev) {
    if (!p) return 1;
    return download(p, GET_CUR, p->bufs.X[0], p->bufs.X[1], X, dev, p->T * p->udims.n_x, p->mapped ? &p->map.x : nullptr, p->T);
}
static int get_U(ilqr_problem* p, double* U, bool dev) {
    if (!p) return 1;
    return download(p, GET_CUR, p->bufs.U[0], p->bufs.U[1], U, dev, (p->T - 1) * p->udims.n_u, p->mapped ? &p->map.u : nullptr, p->T - 1);
}
extern "C" int ilqr_problem_get_X(ilqr_problem* p, double* X) { return get_X(p, X, false); }
extern "C" int ilqr_problem_get_U(ilqr_problem* p, double* U) { return get_U(p, U, false); }
extern "C" int ilqr_problem_get_X_dev(ilqr_problem* p, double* X) { return get_X(p, X, true); }
extern "C" int ilqr_problem_get_U_dev(ilqr_problem* p, double* U) { return get_U(p, U, true); }
static int get_gains(ilqr_problem* p, double* K, double* d) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    double* dst = K ? K : d;
    if (!dst) return fail(c, "null output pointer");
    const int T1 = p->T - 1, nu = p->dims.n_u, nx = p->dims.n_x;
    const size_t n = (size_t)p->B * T1 * p->udims.n_u * (K ? p->udims.n_x : 1);
    if (p->staging.reserve(c, n)) return 1;
    if (p->mapped)
        launch_get_gains_map(p->bufs.KD, p->bufs.kd_sym, p->bufs.alpha, p->bufs.iters, K ? p->staging.ptr : nullptr, K ? nullptr : p->staging.ptr, p->B, p->Bp, T1, p->map,
                             c->stream);
    else
        launch_get_gains(p->bufs.KD, p->bufs.kd_sym, p->bufs.alpha, p->bufs.iters, K ? p->staging.ptr : nullptr, K ? nullptr : p->staging.ptr, p->B, p->Bp, T1, nu, nx,
                         c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(dst, p->staging.ptr, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
// ---- receding horizon / tracking
extern "C" int ilqr_problem_warm_start(ilqr_problem* p, int shift) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    if (!p->has_state || !p->has_controls) return fail(c, "warm start needs a previous solve (set_init_state, set_controls, solve)");
    if (shift < 0 || shift >= p->T) return fail(c, "shift must be in [0, T)");
    p->has_gains = p->has_plan = false;  // U0 and the start state change
    HIPCHK(c, hipSetDevice(c->device));
    launch_warm_start(p->bufs, const_cast<double*>(p->bufs.U0), const_cast<double*>(p->bufs.q0), const_cast<double*>(p->bufs.dq0), shift, p->B, p->T,
                      p->dims.n_x, p->dims.n_u, p->desc.nb_deriv, c->stream);
    HIPCHK(c, hipGetLastError());
    return 0;
}
static int track(ilqr_problem* p, int k, const double* x_meas, int with_ff, double* u_out, bool dev) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    if (!x_meas || !u_out) return fail(c, "null pointer");
    if (k < 0 || k >= p->T - 1) return fail(c, "timestep outside [0, T-2]");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nxb = (size_t)p->B * p->udims.n_x, nub = (size_t)p->B * p->udims.n_u;
    const double* xs = x_meas;
    double* us = u_out;
    if (!dev) {
        if (p->staging.reserve(c, nxb + nub)) return 1;
        HIPCHK(c, hipMemcpyAsync(p->staging.ptr, x_meas, nxb * sizeof(double), hipMemcpyHostToDevice, c->stream));
        xs = p->staging.ptr;
        us = p->staging.ptr + nxb;
    }
    if (p->mapped) launch_track_map(p->bufs, xs, k, with_ff, us, p->B, p->map, c->stream);
    else launch_track(p->bufs, xs, k, with_ff, us, p->B, p->dims.n_x, p->dims.n_u, c->stream);
    HIPCHK(c, hipGetLastError());
    if (!dev) {
        HIPCHK(c, hipMemcpyAsync(u_out, us, nub * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}
extern "C" int ilqr_problem_track(ilqr_problem* p, int k, const double* x_meas, int with_feedforward, double* u_out) {
    return track(p, k, x_meas, with_feedforward, u_out, false);
}
extern "C" int ilqr_problem_track_dev(ilqr_problem* p, int k, const double* x_meas, int with_feedforward, double* u_out) {
    return track(p, k, x_meas, with_feedforward, u_out, true);
}

// ------------------------------------------------------------------------------------------------ closed loop
// Closed loop of the tracking law on the last plan (ilqr_closed_loop.hpp): n_samples executions per instance.  Which kernel runs is decided by
// plan_closed_loop; chains of fewer than 7 joints take the generic kernel's mapped variant.  Each of the six entry points fills a ClRequest, and
// closed_loop does its jobs in turn: cl_check (every refusal), cl_bind (the memory the kernels see every array in), cl_launch and, for host
// pointers, ClStaging::fetch.
struct ClRequest {
    int S = 0;
    const double *x0 = nullptr, *w = nullptr;  // [B][S][n_x], [B][S][T-1][n_x] or null
    int with_ff = 0;
    double *cost = nullptr, *X = nullptr, *U = nullptr;
    bool dev = false;  // every array is a device pointer, and the call is asynchronous
    // draw the disturbances (ilqr_noise.hpp).  The entry point's own flag, not "a noise is given": ilqr_problem_closed_loop_noise sets it always
    // (and a null noise is refused), ilqr_problem_closed_loop_report where a noise is given
    bool noisy = false;
    const ilqr_noise* noise = nullptr;
    double *stats = nullptr, *w_out = nullptr;
    // ilqr_problem_closed_loop_report: the same rollout with the states of the step-table entries and the limit share kept (ClArgs::kpx,
    // lim_cost), then k_closed_loop_kp_err and the two reductions; cost may be null
    bool report = false;
    const ilqr_cl_tol* tol = nullptr;
    const ilqr_cl_report* out = nullptr;
    // ilqr_problem_closed_loop_report_con: a report (out may be null) with the constraint rows judged in the rollout (ClArgs::con_max,
    // con_steps), then the two reductions
    bool con = false;
    double con_tol = 0;
    const ilqr_cl_con* co = nullptr;
    ilqr_cl_report rep() const { return (report && out) ? *out : ilqr_cl_report{}; }
    ilqr_cl_con cons() const { return (con && co) ? *co : ilqr_cl_con{}; }
};

// Every refusal, before anything is allocated or launched; the caller sees the first condition that fails.
static int cl_check(const ilqr_problem* p, const ClRequest& rq) {
    ilqr_ctx* c = p->ctx;
    if (!p->has_gains)
        return fail(c, "closed loop needs the gains of a Riccati solve (ilqr_solve_recursive or ilqr_solve_al with nb_iter >= 1) or of ilqr_problem_gains since the problem's inputs last changed");
    if (rq.S < 1) return fail(c, "n_samples must be >= 1");
    const int T = p->T, nxu = p->udims.n_x, nuu = p->udims.n_u;
    if (rq.noisy) {
        const ilqr_noise* nz = rq.noise;
        if (!nz) return fail(c, "noise is a null pointer");
        for (int i = 0; i < nxu; i++)
            if (!(nz->sigma_w[i] >= 0) || !std::isfinite(nz->sigma_w[i]) || !(nz->sigma_x0[i] >= 0) || !std::isfinite(nz->sigma_x0[i]))
                return fail(c, "closed loop: every sigma_w and sigma_x0 must be finite and >= 0");
        if (!rq.report && !rq.cost && !rq.stats) return fail(c, "cost and stats are both null pointers");
        if ((unsigned long long)nz->instance_offset + (unsigned long long)p->B > (1ull << 32) ||
            (unsigned long long)nz->sample_offset + (unsigned long long)rq.S > (1ull << 32))
            return fail(c, "closed loop: instance_offset + B or sample_offset + n_samples exceeds 2^32 (the generator's counter)");
    } else if (!rq.report && !rq.cost) return fail(c, "cost is a null pointer");
    if (rq.report) {
        const ilqr_cl_tol* tol = rq.tol;
        const ilqr_cl_report rpv = rq.rep();
        const ilqr_cl_report* out = &rpv;
        const bool no_out = !out->kp_err && !out->kp_stats && !out->lim_cost && !out->outcome;
        if (rq.noisy && rq.w) return fail(c, "closed loop report: noise and w are both given (the draw or the caller's disturbances, not both)");
        if (!rq.con && no_out) return fail(c, "closed loop report: every report output is a null pointer");
        if (tol) {
            bool nan = std::isnan(tol->lim_tol);
            for (int k = 0; k < p->hdesc.steps.kp[p->hdesc.steps.n]; k++)
                for (int g = 0; g < ILQR_KP_ERR; g++) nan = nan || std::isnan(tol->kp_tol[k][g]);
            if (nan) return fail(c, "closed loop report: a tolerance is NaN");
            if (tol->lim_tol < 0) return fail(c, "closed loop report: lim_tol must be >= 0");
        } else if (out->kp_stats || out->outcome)
            return fail(c, "closed loop report: tol is a null pointer while kp_stats or outcome is asked for");
        if (rq.con) {
            const ilqr_cl_con oc = rq.cons();
            if (p->bufs.m <= 0) return fail(c, "closed loop report con: no constraints set");
            if (std::isnan(rq.con_tol)) return fail(c, "closed loop report con: con_tol is NaN");
            if (oc.outcome_con && !tol) return fail(c, "closed loop report con: tol is a null pointer while outcome_con is asked for");
            if (no_out && !oc.con_max && !oc.con_steps && !oc.con_stats && !oc.outcome_con)
                return fail(c, "closed loop report con: con and out both ask for nothing");
        }
    }
    // the kernels address the caller's arrays with 32-bit element offsets
    const size_t n = (size_t)p->B * rq.S;
    if ((rq.noisy || rq.report) && !rq.X && !rq.U && !rq.w_out && !rq.w) {  // no per-step array: x0 and cost are the longest
        if (n * (size_t)nxu >= ((size_t)1 << 31))
            return fail(c, "closed loop: B * n_samples * n_x overflows the kernels' 32-bit offsets (split the samples over several calls)");
    } else if (n * T * (size_t)(nxu > nuu ? nxu : nuu) >= ((size_t)1 << 31))
        return fail(c, "closed loop: B * n_samples * T * n_x overflows the kernels' 32-bit offsets (split the samples over several calls)");
    return 0;
}

// The staging area of a host-pointer call, laid out by one cursor: every slice is the next n doubles.  cl_bind walks it twice, first without a
// base, which gives the size to reserve (nothing is copied or noted), then over the reserved area: the size cannot disagree with the walk.
struct ClStaging {
    ilqr_ctx* c;
    double* base;
    size_t used = 0;
    bool failed = false;  // a copy in has failed: the context holds the error
    struct Back { double* host; const double* dev; size_t n; } back[13];  // at most cost, stats, w_out, X, U, the four report outputs and the four of the constraints
    int n_back = 0;
    int copy(void* dst, const void* src, size_t n, hipMemcpyKind kind) { HIPCHK(c, hipMemcpyAsync(dst, src, n * sizeof(double), kind, c->stream)); return 0; }
    double* take(size_t n) { used += n; return base ? base + (used - n) : nullptr; }
    const double* take_in(const double* host, size_t n) {  // ... filled with the caller's input
        double* s = take(n);
        if (base && copy(s, host, n, hipMemcpyHostToDevice)) failed = true;
        return s;
    }
    double* take_out(double* host, size_t n) {  // ... which fetch copies to `host`, where there is one
        double* s = take(n);
        if (base && host && n) back[n_back++] = {host, s, n};
        return s;
    }
    int fetch() {
        for (int i = 0; i < n_back; i++)
            if (copy(back[i].host, back[i].dev, back[i].n, hipMemcpyDeviceToHost)) return 1;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    }
};

struct ClBound {  // what the kernels see
    ClArgs a;
    double* stats = nullptr;  // the device side of stats
    ilqr_cl_report dr = {};   // ... and of the four report outputs
    ilqr_cl_con dc = {};      // ... and of the four outputs of the constraints
};

// Per array: the caller's device pointer, a slice of staging (host pointers), or a workspace of the problem (what the caller does not ask for
// but a kernel reads).  rq has passed cl_check.
static int cl_bind(ilqr_problem* p, const ClRequest& rq, const ClosedLoopPlan& pl, ClStaging& stg, ClBound& b) {
    ilqr_ctx* c = p->ctx;
    const int T = p->T, nxu = p->udims.n_x, nuu = p->udims.n_u;
    const size_t n = (size_t)p->B * rq.S;
    const ilqr_cl_report rp = rq.rep();
    const ilqr_cl_con oc = rq.cons();
    const int n_kp = p->hdesc.steps.kp[p->hdesc.steps.n];
    // kp_err feeds both reductions, lim_cost the outcome; outcome_con reads what outcome reads
    const bool want_ke = rp.kp_err || rp.kp_stats || rp.outcome || oc.outcome_con, want_lc = rp.lim_cost || rp.outcome || oc.outcome_con;
    const size_t n_ke = want_ke ? n * n_kp * ILQR_KP_ERR : 0, n_lc = want_lc ? n : 0;
    // con_max switches the kernels' constraint code on, so it exists for any of the four; con_steps feeds con_stats
    const bool want_cm = oc.con_max || oc.con_steps || oc.con_stats || oc.outcome_con, want_cs = oc.con_steps || oc.con_stats;
    const size_t n_cm = want_cm ? n : 0, n_cs = want_cs ? n : 0;
    if (pl.coop || rq.report)  // the report reads the states of the step-table entries from either kernel
        if (p->cl_kpx.reserve(c, (size_t)(p->hdesc.steps.n > 0 ? p->hdesc.steps.n : 1) * (p->dims.n_x + p->dims.n_u) * n)) return 1;
    ClArgs& a = b.a;
    a.S = rq.S; a.with_ff = rq.with_ff ? 1 : 0; a.x0 = rq.x0; a.w = rq.w; a.cost = rq.cost; a.X = rq.X; a.U = rq.U; a.w_out = rq.w_out;
    if (rq.noisy) {
        a.noise = 1; a.seed = rq.noise->seed; a.b_off = rq.noise->instance_offset; a.s_off = rq.noise->sample_offset;
        for (int i = 0; i < nxu; i++) { a.sigma_w[i] = rq.noise->sigma_w[i]; a.sigma_x0[i] = rq.noise->sigma_x0[i]; }
    }
    b.stats = rq.stats;
    b.dr = rp;
    b.dc = oc;
    if (rq.dev) {
        if (!rq.cost) {  // the per-sample costs live in a workspace: stats and outcome read them there
            if (p->cl_cost.reserve(c, n)) return 1;
            a.cost = p->cl_cost.ptr;
        }
        if (rq.report) {  // kp_err | lim_cost where the caller asks only for their reductions
            const size_t ws_ke = rp.kp_err ? 0 : n_ke, ws_lc = rp.lim_cost ? 0 : n_lc;
            if (p->cl_rep.reserve(c, ws_ke + ws_lc)) return 1;
            if (!rp.kp_err) b.dr.kp_err = p->cl_rep.ptr;
            if (!rp.lim_cost) b.dr.lim_cost = p->cl_rep.ptr + ws_ke;
        }
        if (rq.con) {  // con_max | con_steps likewise
            const size_t ws_cm = oc.con_max ? 0 : n_cm, ws_cs = oc.con_steps ? 0 : n_cs;
            if (p->cl_con_ws.reserve(c, ws_cm + ws_cs)) return 1;
            if (!oc.con_max) b.dc.con_max = p->cl_con_ws.ptr;
            if (!oc.con_steps) b.dc.con_steps = p->cl_con_ws.ptr + ws_cm;
        }
    } else {
        if (rq.x0) a.x0 = stg.take_in(rq.x0, n * nxu);
        if (rq.w) a.w = stg.take_in(rq.w, n * (T - 1) * nxu);
        a.cost = stg.take_out(rq.cost, n);  // always staged: stats and outcome read it
        if (rq.stats) b.stats = stg.take_out(rq.stats, (size_t)p->B * ILQR_CL_STATS);
        if (rq.w_out) a.w_out = stg.take_out(rq.w_out, n * (T - 1) * nxu);
        if (rq.X) a.X = stg.take_out(rq.X, n * T * nxu);
        if (rq.U) a.U = stg.take_out(rq.U, n * (T - 1) * nuu);
        if (rq.report) {
            b.dr.kp_err = stg.take_out(rp.kp_err, n_ke);
            b.dr.lim_cost = stg.take_out(rp.lim_cost, n_lc);
            b.dr.kp_stats = stg.take_out(rp.kp_stats, rp.kp_stats ? (size_t)p->B * n_kp * ILQR_KP_STATS : 0);
            b.dr.outcome = stg.take_out(rp.outcome, rp.outcome ? (size_t)p->B * ILQR_CL_OUTCOME : 0);
        }
        if (rq.con) {
            b.dc.con_max = stg.take_out(oc.con_max, n_cm);
            b.dc.con_steps = stg.take_out(oc.con_steps, n_cs);
            b.dc.con_stats = stg.take_out(oc.con_stats, oc.con_stats ? (size_t)p->B * ILQR_CL_CON_STATS : 0);
            b.dc.outcome_con = stg.take_out(oc.outcome_con, oc.outcome_con ? (size_t)p->B * ILQR_CL_OUTCOME_CON : 0);
        }
        if (stg.failed) return 1;
    }
    if (rq.report) { a.kpx = pl.coop ? nullptr : p->cl_kpx.ptr; a.lim_cost = want_lc ? b.dr.lim_cost : nullptr; }
    if (rq.con) { a.con_tol = rq.con_tol; a.con_max = want_cm ? b.dc.con_max : nullptr; a.con_steps = want_cs ? b.dc.con_steps : nullptr; }
    return 0;
}

static void cl_launch(ilqr_problem* p, const ClRequest& rq, const ClosedLoopPlan& pl, const ClBound& b) {
    const int kind = p->desc.kind, nd = p->desc.nb_deriv, B = p->B, S = rq.S, n_kp = p->hdesc.steps.kp[p->hdesc.steps.n];
    hipStream_t st = p->ctx->stream;
    if (pl.coop) launch_closed_loop_coop(kind, nd, p->bufs, b.a, B, pl, p->cl_kpx.ptr, st);
    else launch_closed_loop(kind, nd, p->bufs, b.a, B, p->mapped ? &p->map : nullptr, st);
    if (rq.stats) launch_closed_loop_stats(b.a.cost, B, S, b.stats, st);
    if (!rq.report) return;
    const ilqr_cl_report rp = rq.rep();
    const ilqr_cl_con oc = rq.cons();
    if (rp.kp_err || rp.kp_stats || rp.outcome || oc.outcome_con) launch_closed_loop_kp_err(kind, nd, p->bufs, B, S, n_kp, p->cl_kpx.ptr, b.dr.kp_err, st);
    if (rp.kp_stats) launch_closed_loop_kp_stats(b.dr.kp_err, *rq.tol, B, S, n_kp, b.dr.kp_stats, st);
    if (rp.outcome) launch_closed_loop_outcome(b.a.cost, b.dr.kp_err, b.dr.lim_cost, *rq.tol, B, S, n_kp, b.dr.outcome, st);
    if (oc.con_stats) launch_closed_loop_con_stats(b.dc.con_max, b.dc.con_steps, rq.con_tol, B, S, b.dc.con_stats, st);
    if (oc.outcome_con)
        launch_closed_loop_outcome_con(b.a.cost, b.dr.kp_err, b.dr.lim_cost, b.dc.con_max, *rq.tol, rq.con_tol, B, S, n_kp, b.dc.outcome_con, st);
}

static int closed_loop(ilqr_problem* p, const ClRequest& rq) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    if (cl_check(p, rq)) return 1;
    HIPCHK(c, hipSetDevice(c->device));
    const ClosedLoopPlan pl = plan_closed_loop(p->desc.kind, p->desc.nb_deriv, rq.S, p->B, c->n_simd, c->xc_generic || p->mapped);
    if (pl.coop && !launch_closed_loop_coop) return fail(c, "closed loop: the cooperative kernels are not part of this build (pin the generic kernels)");
    ClBound b;
    if (!rq.dev) {  // the sizing walk
        ClStaging size{c, nullptr};
        if (cl_bind(p, rq, pl, size, b) || p->staging.reserve(c, size.used)) return 1;
    }
    ClStaging stg{c, rq.dev ? nullptr : p->staging.ptr};
    if (cl_bind(p, rq, pl, stg, b)) return 1;
    cl_launch(p, rq, pl, b);
    HIPCHK(c, hipGetLastError());
    return rq.dev ? 0 : stg.fetch();
}

extern "C" int ilqr_problem_closed_loop(ilqr_problem* p, int n_samples, const double* x0, const double* w, int with_feedforward, double* cost, double* X,
                                        double* U) {
    return closed_loop(p, {.S = n_samples, .x0 = x0, .w = w, .with_ff = with_feedforward, .cost = cost, .X = X, .U = U});
}
extern "C" int ilqr_problem_closed_loop_dev(ilqr_problem* p, int n_samples, const double* x0, const double* w, int with_feedforward, double* cost,
                                            double* X, double* U) {
    return closed_loop(p, {.S = n_samples, .x0 = x0, .w = w, .with_ff = with_feedforward, .cost = cost, .X = X, .U = U, .dev = true});
}

extern "C" int ilqr_problem_closed_loop_noise(ilqr_problem* p, int n_samples, const ilqr_noise* noise, const double* x0, int with_feedforward,
                                              double* cost, double* stats, double* X, double* U, double* w_out) {
    return closed_loop(p, {.S = n_samples, .x0 = x0, .with_ff = with_feedforward, .cost = cost, .X = X, .U = U, .noisy = true, .noise = noise,
                           .stats = stats, .w_out = w_out});
}
extern "C" int ilqr_problem_closed_loop_noise_dev(ilqr_problem* p, int n_samples, const ilqr_noise* noise, const double* x0, int with_feedforward,
                                                  double* cost, double* stats, double* X, double* U, double* w_out) {
    return closed_loop(p, {.S = n_samples, .x0 = x0, .with_ff = with_feedforward, .cost = cost, .X = X, .U = U, .dev = true, .noisy = true,
                           .noise = noise, .stats = stats, .w_out = w_out});
}

extern "C" int ilqr_problem_closed_loop_report(ilqr_problem* p, int n_samples, const ilqr_noise* noise, const double* x0, const double* w,
                                               int with_feedforward, const ilqr_cl_tol* tol, double* cost, double* stats, const ilqr_cl_report* out) {
    return closed_loop(p, {.S = n_samples, .x0 = x0, .w = w, .with_ff = with_feedforward, .cost = cost, .noisy = noise != nullptr, .noise = noise,
                           .stats = stats, .report = true, .tol = tol, .out = out});
}
extern "C" int ilqr_problem_closed_loop_report_dev(ilqr_problem* p, int n_samples, const ilqr_noise* noise, const double* x0, const double* w,
                                                   int with_feedforward, const ilqr_cl_tol* tol, double* cost, double* stats, const ilqr_cl_report* out) {
    return closed_loop(p, {.S = n_samples, .x0 = x0, .w = w, .with_ff = with_feedforward, .cost = cost, .dev = true, .noisy = noise != nullptr,
                           .noise = noise, .stats = stats, .report = true, .tol = tol, .out = out});
}

extern "C" int ilqr_problem_closed_loop_report_con(ilqr_problem* p, int n_samples, const ilqr_noise* noise, const double* x0, const double* w,
                                                   int with_feedforward, const ilqr_cl_tol* tol, double* cost, double* stats,
                                                   const ilqr_cl_report* out, double con_tol, const ilqr_cl_con* con) {
    return closed_loop(p, {.S = n_samples, .x0 = x0, .w = w, .with_ff = with_feedforward, .cost = cost, .noisy = noise != nullptr, .noise = noise,
                           .stats = stats, .report = true, .tol = tol, .out = out, .con = true, .con_tol = con_tol, .co = con});
}
extern "C" int ilqr_problem_closed_loop_report_con_dev(ilqr_problem* p, int n_samples, const ilqr_noise* noise, const double* x0, const double* w,
                                                       int with_feedforward, const ilqr_cl_tol* tol, double* cost, double* stats,
                                                       const ilqr_cl_report* out, double con_tol, const ilqr_cl_con* con) {
    return closed_loop(p, {.S = n_samples, .x0 = x0, .w = w, .with_ff = with_feedforward, .cost = cost, .dev = true, .noisy = noise != nullptr,
                           .noise = noise, .stats = stats, .report = true, .tol = tol, .out = out, .con = true, .con_tol = con_tol, .co = con});
}

// The covariance of that closed loop, propagated analytically (ilqr_closed_loop_cov.hpp).  Which kernel runs is decided by plan_closed_loop_cov.
// kp_var is formed from kp_Sigma by a kernel of its own, so kp_Sigma always exists where kp_var is asked for: the caller's array, a slice of
// staging, or the problem's workspace.
// with_con: ilqr_problem_closed_loop_cov_con -- `out_` may be null, and the kernels also read the constraint rows off Sigma_k (con).
static int closed_loop_cov(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out_, bool dev, bool with_con = false,
                           const ilqr_cl_cov_con* con = nullptr) {
    if (!p) return 1;
    const ilqr_cl_cov none = {};
    const ilqr_cl_cov* out = (with_con && !out_) ? &none : out_;
    const ilqr_cl_cov_con oc = (with_con && con) ? *con : ilqr_cl_cov_con{};
    ilqr_ctx* c = p->ctx;
    const int T = p->T, nxu = p->udims.n_x, nuu = p->udims.n_u, B = p->B, n_kp = p->hdesc.steps.kp[p->hdesc.steps.n];
    for (int i = 0; i < nxu; i++)
        for (const double* sg : {sigma_w, sigma_x0})
            if (sg && (!(sg[i] >= 0) || !std::isfinite(sg[i]))) return fail(c, "closed loop: every sigma_w and sigma_x0 must be finite and >= 0");
    const bool no_out = !out || (!out->Sigma && !out->kp_Sigma && !out->kp_var && !out->u_var && !out->lim_z);
    if (!with_con && no_out) return fail(c, "closed loop cov: every output is a null pointer");
    const size_t nn = (size_t)nxu * nxu, n_S = (size_t)B * T * nn, n_kS = (size_t)B * n_kp * nn;
    if (const char* why = cl_cov_size_refusal(B, T, n_kp, nxu, out->Sigma != nullptr, out->kp_Sigma != nullptr)) return fail(c, why);
    if (!p->has_gains)   // (behind the bounds on the call itself: those do not depend on the state of the problem)
        return fail(c, "closed loop needs the gains of a Riccati solve (ilqr_solve_recursive or ilqr_solve_al with nb_iter >= 1) or of ilqr_problem_gains since the problem's inputs last changed");
    if (with_con) {
        if (p->bufs.m <= 0) return fail(c, "closed loop cov con: no constraints set");
        if (no_out && !oc.con_var && !oc.con_z) return fail(c, "closed loop cov con: con and out both ask for nothing");
    }
    const size_t n_cv = (size_t)B * (T - 1) * (with_con ? p->bufs.m : 0);
    HIPCHK(c, hipSetDevice(c->device));
    const ClosedLoopCovPlan pl = plan_closed_loop_cov(p->desc.kind, p->desc.nb_deriv, B, c->n_simd, c->xc_generic || p->mapped);
    if (pl.rows && !launch_closed_loop_cov_rows) return fail(c, "closed loop cov: the row kernel is not part of this build (pin the generic kernels)");

    ClCovArgs a;
    for (int i = 0; i < p->dims.n_x; i++) {
        const int iu = p->mapped ? p->map.x.usr[i] : i;
        if (iu < 0) continue;
        a.sw2[i] = sigma_w ? sigma_w[iu] * sigma_w[iu] : 0.0;
        a.sx02[i] = sigma_x0 ? sigma_x0[iu] * sigma_x0[iu] : 0.0;
    }
    const bool want_kS = (out->kp_Sigma || out->kp_var) && n_kp > 0;
    const size_t n_kv = (size_t)B * n_kp * ILQR_CL_COV_KP, n_uv = (size_t)B * (T - 1) * nuu;
    double* kp_var = out->kp_var;
    a.Sigma = out->Sigma; a.kp_Sigma = out->kp_Sigma; a.u_var = out->u_var; a.lim_z = out->lim_z;
    a.con_var = oc.con_var; a.con_z = oc.con_z;
    auto bind = [&](ClStaging& stg) {  // the staging slices of a host-pointer call (ClStaging: first the sizing walk, then the real one)
        if (out->Sigma) a.Sigma = stg.take_out(out->Sigma, n_S);
        a.kp_Sigma = want_kS ? stg.take_out(out->kp_Sigma, n_kS) : nullptr;
        if (out->kp_var) kp_var = stg.take_out(out->kp_var, n_kv);
        if (out->u_var) a.u_var = stg.take_out(out->u_var, n_uv);
        if (out->lim_z) a.lim_z = stg.take_out(out->lim_z, (size_t)B);
        if (oc.con_var) a.con_var = stg.take_out(oc.con_var, n_cv);
        if (oc.con_z) a.con_z = stg.take_out(oc.con_z, (size_t)B);
    };
    if (!dev) {
        ClStaging size{c, nullptr};
        bind(size);
        if (p->staging.reserve(c, size.used)) return 1;
    } else if (want_kS && !out->kp_Sigma) {
        if (p->cl_cov_kps.reserve(c, n_kS)) return 1;
        a.kp_Sigma = p->cl_cov_kps.ptr;
    }
    ClStaging stg{c, dev ? nullptr : p->staging.ptr};
    if (!dev) bind(stg);
    if (!want_kS) a.kp_Sigma = nullptr;
    if (!pl.rows) {
        if (p->cl_cov_ws.reserve(c, (size_t)cl_cov_ws_entries(p->desc.kind, p->desc.nb_deriv) * p->Bp)) return 1;
        a.ws = p->cl_cov_ws.ptr;
    }
    const int kind = p->desc.kind, nd = p->desc.nb_deriv;
    if (pl.rows) launch_closed_loop_cov_rows(kind, nd, p->bufs, a, B, c->stream);
    else launch_closed_loop_cov(kind, nd, p->bufs, a, B, p->mapped ? &p->map : nullptr, c->stream);
    if (out->kp_var) launch_closed_loop_cov_kp(kind, nd, p->bufs, B, n_kp, p->mapped ? p->map.dof : DOF, a.kp_Sigma, kp_var, c->stream);
    HIPCHK(c, hipGetLastError());
    return dev ? 0 : stg.fetch();
}
extern "C" int ilqr_problem_closed_loop_cov(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out) {
    return closed_loop_cov(p, sigma_w, sigma_x0, out, false);
}
extern "C" int ilqr_problem_closed_loop_cov_dev(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out) {
    return closed_loop_cov(p, sigma_w, sigma_x0, out, true);
}

extern "C" int ilqr_problem_closed_loop_cov_con(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out,
                                                const ilqr_cl_cov_con* con) {
    return closed_loop_cov(p, sigma_w, sigma_x0, out, false, true, con);
}
extern "C" int ilqr_problem_closed_loop_cov_con_dev(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out,
                                                    const ilqr_cl_cov_con* con) {
    return closed_loop_cov(p, sigma_w, sigma_x0, out, true, true, con);
}

extern "C" int ilqr_problem_get_K(ilqr_problem* p, double* K) { return get_gains(p, K, nullptr); }
extern "C" int ilqr_problem_get_d(ilqr_problem* p, double* d) { return get_gains(p, nullptr, d); }
extern "C" int ilqr_problem_get_cost(ilqr_problem* p, double* cost) { return p ? download(p, GET_PLAIN, p->bufs.cost, nullptr, cost, false, 1) : 1; }
extern "C" int ilqr_problem_get_cost_dev(ilqr_problem* p, double* cost) { return p ? download(p, GET_PLAIN, p->bufs.cost, nullptr, cost, true, 1) : 1; }
extern "C" int ilqr_problem_get_alpha(ilqr_problem* p, double* alpha) { return p ? download(p, GET_PLAIN, p->bufs.alpha, nullptr, alpha, false, 1) : 1; }
extern "C" int ilqr_problem_get_lambda(ilqr_problem* p, double* lam) {
    if (!p) return 1;
    if (p->bufs.m <= 0) return fail(p->ctx, "no constraints set");
    return download(p, GET_PLAIN, p->bufs.lambda, nullptr, lam, false, (p->T - 1) * p->bufs.m);
}

static int get_ints(ilqr_problem* p, const int* src, int* dst) {
    if (!p) return 1;
    if (!dst) return fail(p->ctx, "null output pointer");
    HIPCHK(p->ctx, hipMemcpyAsync(dst, src, sizeof(int) * p->B, hipMemcpyDeviceToHost, p->ctx->stream));
    HIPCHK(p->ctx, hipStreamSynchronize(p->ctx->stream));
    return 0;
}
extern "C" int ilqr_problem_get_iters(ilqr_problem* p, int* iters) { return get_ints(p, p ? p->bufs.iters : nullptr, iters); }
extern "C" int ilqr_problem_get_status(ilqr_problem* p, int* status) { return get_ints(p, p ? p->bufs.status : nullptr, status); }

extern "C" int ilqr_problem_get_trace(ilqr_problem* p, double* ct, double* at, int nb_iter) {
    if (!p) return 1;
    if (nb_iter <= 0 || nb_iter > p->last_nb_iter) return fail(p->ctx, "nb_iter exceeds the last solve's iteration count");
    if (ct && download(p, GET_PLAIN, p->bufs.cost_trace, nullptr, ct, false, nb_iter)) return 1;
    if (at && download(p, GET_PLAIN, p->bufs.alpha_trace, nullptr, at, false, nb_iter)) return 1;
    return 0;
}

extern "C" int ilqr_problem_get_fX(ilqr_problem* p, double* fX) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    if (!fX) return fail(c, "null output pointer");
    const size_t n = (size_t)p->B * p->T * p->dims.n_f;
    if (p->staging.reserve(c, n)) return 1;
    {
        ProfScope ps(c, ILQR_PROF_OTHER);
        launch_fx_all(p->desc.kind, p->desc.nb_deriv, p->bufs, p->B, p->T, p->staging.ptr, c->stream);
    }
    prof_mark(c, -1);
    HIPCHK(c, hipGetLastError());
    const bool narrow = p->udims.n_f != p->dims.n_f;  // f(x) = x of a joint-space system of fewer than 7 joints: the state map
    std::vector<double> wide(narrow ? n : 0);
    HIPCHK(c, hipMemcpyAsync(narrow ? wide.data() : fX, p->staging.ptr, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (narrow) {
        const IndexMap& mx = p->map.x;
        for (size_t r = 0; r < (size_t)p->B * p->T; r++)
            for (int i = 0; i < mx.n_user; i++) fX[r * mx.n_user + i] = wide[r * mx.n_dev + mx.dev[i]];
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ multi-start
// The calls that join instances (include/ilqr_hip.h "multi-start"): every refusal first, then the launches of ilqr_multistart.hpp on the context's
// stream, charged to ILQR_PROF_OTHER.  Host forms stage their int arrays in ms_idx / ms_out and their doubles in `staging`, and synchronise.

static int ms_groups(ilqr_ctx* c, const char* fn, int B, int S) {
    if (S < 1) return fail(c, std::string(fn) + ": group_size must be >= 1 (got " + std::to_string(S) + ")");
    if (B % S != 0) return fail(c, std::string(fn) + ": the batch (" + std::to_string(B) + ") is not a multiple of group_size (" + std::to_string(S) + ")");
    return 0;
}
// n ints at the front of a scratch of doubles
static int ms_ints(ilqr_ctx* c, DevScratch& s, size_t n, int** out) {
    if (s.reserve(c, (n + 1) / 2 + 1)) return 1;
    *out = (int*)s.ptr;
    return 0;
}
// the index of a call as the kernels read it: the caller's device pointer, or the host array checked against 0 .. B_src-1 and uploaded
static int ms_index(ilqr_problem* owner, const char* fn, const int* index, int n, int B_src, bool dev, const int** out) {
    ilqr_ctx* c = owner->ctx;
    if (dev) { *out = index; return 0; }
    for (int i = 0; i < n; i++)
        if (index[i] < 0 || index[i] >= B_src)
            return fail(c, std::string(fn) + ": index[" + std::to_string(i) + "] = " + std::to_string(index[i]) + " is outside 0 .. " + std::to_string(B_src - 1));
    int* d = nullptr;
    if (ms_ints(c, owner->ms_idx, (size_t)n, &d)) return 1;
    HIPCHK(c, hipMemcpyAsync(d, index, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    *out = d;
    return 0;
}

static int adopt(ilqr_problem* dst, ilqr_problem* src, const int* index, int what, bool dev) {
    if (!dst) return 1;
    ilqr_ctx* c = dst->ctx;
    const char* fn = "ilqr_problem_adopt";
    if (!src) return fail(c, "ilqr_problem_adopt: src is a null pointer");
    if (!index) return fail(c, "ilqr_problem_adopt: index is a null pointer");
    if (src->ctx != c) return fail(c, "ilqr_problem_adopt: both problems must belong to one context");
    if (dst == src) return fail(c, "ilqr_problem_adopt: dst and src are the same problem");
    const ilqr_problem_desc &dd = dst->desc, &sd = src->desc;
    if (dd.kind != sd.kind) return fail(c, "ilqr_problem_adopt: the problems differ in kind (" + std::to_string(dd.kind) + " and " + std::to_string(sd.kind) + ")");
    if (dd.nb_deriv != sd.nb_deriv) return fail(c, "ilqr_problem_adopt: the problems differ in nb_deriv (" + std::to_string(dd.nb_deriv) + " and " + std::to_string(sd.nb_deriv) + ")");
    if (dd.dof != sd.dof) return fail(c, "ilqr_problem_adopt: the problems differ in dof (" + std::to_string(dd.dof) + " and " + std::to_string(sd.dof) + ")");
    if (dd.horizon != sd.horizon) return fail(c, "ilqr_problem_adopt: the problems differ in horizon (" + std::to_string(dd.horizon) + " and " + std::to_string(sd.horizon) + ")");
    if (dd.n_kp != sd.n_kp) return fail(c, "ilqr_problem_adopt: the problems differ in n_kp (" + std::to_string(dd.n_kp) + " and " + std::to_string(sd.n_kp) + ")");
    if (what & ILQR_ADOPT_TARGETS)   // a joint-space keypoint's target rows are laid out as a state, a pose keypoint's as f(x): the rows are copied as they are
        for (int k = 0; k < dd.n_kp; k++)
            if ((dd.kp_joint[k] != 0) != (sd.kp_joint[k] != 0))
                return fail(c, "ilqr_problem_adopt: ILQR_ADOPT_TARGETS needs equal kp_joint flags (keypoint " + std::to_string(k) + " is a joint-space keypoint in one problem only)");
    const int all = ILQR_ADOPT_STATE | ILQR_ADOPT_TARGETS | ILQR_ADOPT_CONTROLS0 | ILQR_ADOPT_CONTROLS | ILQR_ADOPT_MULTIPLIERS;
    if (what == 0 || (what & ~all)) return fail(c, "ilqr_problem_adopt: `what` must be a combination of the ILQR_ADOPT_* bits (got " + std::to_string(what) + ")");
    if ((what & ILQR_ADOPT_CONTROLS0) && (what & ILQR_ADOPT_CONTROLS))
        return fail(c, "ilqr_problem_adopt: ILQR_ADOPT_CONTROLS0 and ILQR_ADOPT_CONTROLS both name dst's U0: give one of them");
    if ((what & ILQR_ADOPT_STATE) && !src->has_state) return fail(c, "ilqr_problem_adopt: ILQR_ADOPT_STATE needs a start state in src (ilqr_problem_set_init_state)");
    if ((what & ILQR_ADOPT_CONTROLS0) && !src->has_controls) return fail(c, "ilqr_problem_adopt: ILQR_ADOPT_CONTROLS0 needs controls in src (ilqr_problem_set_controls)");
    if ((what & ILQR_ADOPT_CONTROLS) && !src->has_plan)
        return fail(c, "ilqr_problem_adopt: ILQR_ADOPT_CONTROLS needs a plan in src: run a solver since its inputs last changed");
    if (what & ILQR_ADOPT_MULTIPLIERS) {
        if (src->bufs.m <= 0 || dst->bufs.m <= 0) return fail(c, "ilqr_problem_adopt: ILQR_ADOPT_MULTIPLIERS needs constraint rows in both problems (ilqr_problem_set_constraints)");
        if (src->bufs.m != dst->bufs.m || src->bufs.per_step != dst->bufs.per_step)
            return fail(c, "ilqr_problem_adopt: ILQR_ADOPT_MULTIPLIERS needs rows of equal m and per_step (dst " + std::to_string(dst->bufs.m) + ", " + std::to_string(dst->bufs.per_step) +
                               "; src " + std::to_string(src->bufs.m) + ", " + std::to_string(src->bufs.per_step) + ")");
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int* idx = nullptr;
    if (ms_index(dst, fn, index, dst->B, src->B, dev, &idx)) return 1;
    dst->has_gains = dst->has_plan = false;
    const int T = dst->T, NU = dst->dims.n_u, NF = dst->dims.n_f;
    const Bufs &sb = src->bufs, &db = dst->bufs;
    hipStream_t st = c->stream;
    auto rows = [&](const double* s0, const double* s1, const int* cur, const double* to, int n) {
        ProfScope ps(c, ILQR_PROF_OTHER);
        launch_adopt_rows(s0, s1, cur, idx, const_cast<double*>(to), n, dst->B, dst->Bp, src->B, src->Bp, st);
    };
    if (what & ILQR_ADOPT_STATE) {
        rows(sb.q0, nullptr, nullptr, db.q0, DOF);
        rows(sb.dq0, nullptr, nullptr, db.dq0, DOF);
    }
    if (what & ILQR_ADOPT_TARGETS) rows(sb.kp_tg, nullptr, nullptr, db.kp_tg, dd.n_kp * NF);
    if (what & ILQR_ADOPT_CONTROLS0) rows(sb.U0, nullptr, nullptr, db.U0, (T - 1) * NU);
    if (what & ILQR_ADOPT_CONTROLS) rows(sb.U[0], sb.U[1], sb.cur, db.U0, (T - 1) * NU);
    if (what & ILQR_ADOPT_MULTIPLIERS) rows(sb.lambda, nullptr, nullptr, db.lambda, (T - 1) * db.m);
    HIPCHK(c, hipGetLastError());
    prof_mark(c, -1);
    if (what & ILQR_ADOPT_STATE) dst->has_state = true;
    if (what & (ILQR_ADOPT_CONTROLS0 | ILQR_ADOPT_CONTROLS)) { dst->has_controls = true; dst->u0_zero = false; }
    if (!dev) HIPCHK(c, hipStreamSynchronize(c->stream));  // the index array is the caller's
    return 0;
}
extern "C" int ilqr_problem_adopt(ilqr_problem* dst, ilqr_problem* src, const int* index, int what) { return adopt(dst, src, index, what, false); }
extern "C" int ilqr_problem_adopt_dev(ilqr_problem* dst, ilqr_problem* src, const int* index, int what) { return adopt(dst, src, index, what, true); }

extern "C" int ilqr_problem_spread_controls(ilqr_problem* p, int group_size, const ilqr_seeds* seeds) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    const char* fn = "ilqr_problem_spread_controls";
    if (ms_groups(c, fn, p->B, group_size)) return 1;
    if (!seeds) return fail(c, "ilqr_problem_spread_controls: seeds is a null pointer");
    if (!p->has_controls) return fail(c, "ilqr_problem_spread_controls needs controls: call ilqr_problem_set_controls (or ilqr_problem_adopt) first");
    for (int i = 0; i < p->udims.n_u; i++)
        if (!(seeds->sigma_u[i] >= 0) || !std::isfinite(seeds->sigma_u[i]))
            return fail(c, "ilqr_problem_spread_controls: every sigma_u must be finite and >= 0 (sigma_u[" + std::to_string(i) + "] = " + std::to_string(seeds->sigma_u[i]) + ")");
    const int G = p->B / group_size;
    if ((unsigned long long)seeds->group_offset + (unsigned long long)G > (1ull << 32) ||
        (unsigned long long)seeds->member_offset + (unsigned long long)group_size > (1ull << 32))
        return fail(c, "ilqr_problem_spread_controls: group_offset + G or member_offset + group_size exceeds 2^32 (the generator's counter)");
    HIPCHK(c, hipSetDevice(c->device));
    p->has_gains = p->has_plan = false;
    p->u0_zero = false;
    {
        ProfScope ps(c, ILQR_PROF_OTHER);
        launch_spread_controls(const_cast<double*>(p->bufs.U0), p->B, p->Bp, p->T - 1, group_size, *seeds, p->map.u, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    prof_mark(c, -1);
    return 0;
}
extern "C" int ilqr_problem_spread_controls_dev(ilqr_problem* p, int group_size, const ilqr_seeds* seeds) {
    return ilqr_problem_spread_controls(p, group_size, seeds);
}

static int select_groups(ilqr_problem* p, int S, const double* score, const int* eligible, int* winner, double* best, int* n_cand, bool dev) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    const char* fn = "ilqr_problem_select";
    if (ms_groups(c, fn, p->B, S)) return 1;
    if (!winner && !best && !n_cand) return fail(c, "ilqr_problem_select: winner, best and n_candidates are all null pointers");
    if (!p->has_plan) return fail(c, "ilqr_problem_select needs a plan: run a solver since the problem's inputs last changed");
    HIPCHK(c, hipSetDevice(c->device));
    const int B = p->B, G = B / S;
    const double* dscore = score ? score : p->bufs.cost;
    const int* delig = eligible;
    int *dwin = winner, *dn = n_cand;
    double* dbest = best;
    if (!dev) {
        if (score) {
            if (p->staging.reserve(c, (size_t)B)) return 1;
            HIPCHK(c, hipMemcpyAsync(p->staging.ptr, score, sizeof(double) * (size_t)B, hipMemcpyHostToDevice, c->stream));
            dscore = p->staging.ptr;
        }
        if (eligible) {
            int* e = nullptr;
            if (ms_ints(c, p->ms_idx, (size_t)B, &e)) return 1;
            HIPCHK(c, hipMemcpyAsync(e, eligible, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, c->stream));
            delig = e;
        }
        if (p->ms_out.reserve(c, (size_t)2 * G + 2)) return 1;   // best[G] | winner[G] | n_candidates[G] (ints)
        dbest = p->ms_out.ptr;
        dwin = (int*)(p->ms_out.ptr + G);
        dn = dwin + G;
    }
    {
        ProfScope ps(c, ILQR_PROF_OTHER);
        launch_select_group(dscore, delig, p->bufs.status, G, S, dwin, dbest, dn, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    prof_mark(c, -1);
    if (!dev) {
        if (winner) HIPCHK(c, hipMemcpyAsync(winner, dwin, sizeof(int) * (size_t)G, hipMemcpyDeviceToHost, c->stream));
        if (best) HIPCHK(c, hipMemcpyAsync(best, dbest, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost, c->stream));
        if (n_cand) HIPCHK(c, hipMemcpyAsync(n_cand, dn, sizeof(int) * (size_t)G, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}
extern "C" int ilqr_problem_select(ilqr_problem* p, int group_size, const double* score, const int* eligible, int* winner, double* best, int* n_candidates) {
    return select_groups(p, group_size, score, eligible, winner, best, n_candidates, false);
}
extern "C" int ilqr_problem_select_dev(ilqr_problem* p, int group_size, const double* score, const int* eligible, int* winner, double* best, int* n_candidates) {
    return select_groups(p, group_size, score, eligible, winner, best, n_candidates, true);
}

static int get_at(ilqr_problem* p, int n, const int* index, double* X, double* U, double* cost, int* iters, int* status, bool dev) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    const char* fn = "ilqr_problem_get_at";
    if (n < 1) return fail(c, "ilqr_problem_get_at: n must be >= 1 (got " + std::to_string(n) + ")");
    if (!index) return fail(c, "ilqr_problem_get_at: index is a null pointer");
    if (!X && !U && !cost && !iters && !status) return fail(c, "ilqr_problem_get_at: every output is a null pointer");
    HIPCHK(c, hipSetDevice(c->device));
    const int* idx = nullptr;
    if (ms_index(p, fn, index, n, p->B, dev, &idx)) return 1;
    const int rx = p->T * p->udims.n_x, ru = (p->T - 1) * p->udims.n_u;
    double *dX = X, *dU = U, *dcost = cost;
    int *dit = iters, *dst = status;
    if (!dev) {
        if (p->staging.reserve(c, (size_t)n * ((size_t)rx + ru + 1))) return 1;
        dX = p->staging.ptr;
        dU = dX + (size_t)n * rx;
        dcost = dU + (size_t)n * ru;
        if (ms_ints(c, p->ms_out, (size_t)2 * n, &dit)) return 1;
        dst = dit + n;
    }
    const Bufs& b = p->bufs;
    // one mark per launch that happens
    if (X) { ProfScope ps(c, ILQR_PROF_OTHER); launch_get_at(b.X[0], b.X[1], b.cur, idx, dX, n, p->B, p->Bp, rx, p->mapped ? &p->map.x : nullptr, c->stream); }
    if (U) { ProfScope ps(c, ILQR_PROF_OTHER); launch_get_at(b.U[0], b.U[1], b.cur, idx, dU, n, p->B, p->Bp, ru, p->mapped ? &p->map.u : nullptr, c->stream); }
    if (cost) { ProfScope ps(c, ILQR_PROF_OTHER); launch_get_at(b.cost, nullptr, nullptr, idx, dcost, n, p->B, p->Bp, 1, nullptr, c->stream); }
    if (iters) { ProfScope ps(c, ILQR_PROF_OTHER); launch_get_at_int(b.iters, idx, dit, n, p->B, c->stream); }
    if (status) { ProfScope ps(c, ILQR_PROF_OTHER); launch_get_at_int(b.status, idx, dst, n, p->B, c->stream); }
    HIPCHK(c, hipGetLastError());
    prof_mark(c, -1);
    if (!dev) {
        if (X) HIPCHK(c, hipMemcpyAsync(X, dX, sizeof(double) * (size_t)n * rx, hipMemcpyDeviceToHost, c->stream));
        if (U) HIPCHK(c, hipMemcpyAsync(U, dU, sizeof(double) * (size_t)n * ru, hipMemcpyDeviceToHost, c->stream));
        if (cost) HIPCHK(c, hipMemcpyAsync(cost, dcost, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        if (iters) HIPCHK(c, hipMemcpyAsync(iters, dit, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        if (status) HIPCHK(c, hipMemcpyAsync(status, dst, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}
extern "C" int ilqr_problem_get_at(ilqr_problem* p, int n, const int* index, double* X, double* U, double* cost, int* iters, int* status) {
    return get_at(p, n, index, X, U, cost, iters, status, false);
}
extern "C" int ilqr_problem_get_at_dev(ilqr_problem* p, int n, const int* index, double* X, double* U, double* cost, int* iters, int* status) {
    return get_at(p, n, index, X, U, cost, iters, status, true);
}

// ------------------------------------------------------------------------------------------------ clearance
// include/ilqr_hip.h "clearance": every refusal first, then the three launches of ilqr_clearance.hpp on the context's stream, charged to
// ILQR_PROF_OTHER.  The geometry buffer, the workspace (12 bytes per (trajectory, step)) and the staging of the host forms belong to the context
// and only grow; the geometry is uploaded when it differs from the one the buffer holds.

struct ClrBytes {
    void* ptr = nullptr;
    size_t bytes = 0;
    int reserve(ilqr_ctx* c, size_t n) {
        if (bytes >= n) return 0;
        if (ptr) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(ptr)); ptr = nullptr; bytes = 0; }
        HIPCHK(c, hipMalloc(&ptr, n));
        bytes = n;
        return 0;
    }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
};
struct ClrState {
    ClrGeom host;        // what `geom` holds
    bool have = false;
    ClrBytes geom, ws, io;
};

static void clr_release(ilqr_ctx* c) {
    if (!c->clr) return;
    c->clr->geom.release(); c->clr->ws.release(); c->clr->io.release();
    delete c->clr;
    c->clr = nullptr;
}

// need_out = false: the checks of robot, planes, obstacles and sets alone (ilqr_problem_set_obstacles, which has no outputs and reads no stats_group)
static int clr_check(ilqr_ctx* c, const std::string& fn, const ilqr_problem_desc& d, int n, int T, const ilqr_clr_robot* rb, const ilqr_clr_world* w,
                     const ilqr_clr_out* out, bool dev, bool need_out = true) {
    auto no = [&](const std::string& m) { return fail(c, fn + ": " + m); };
    auto S = [](long long v) { return std::to_string(v); };
    if (!rb) return no("robot is a null pointer");
    if (!w) return no("world is a null pointer");
    if (need_out && !out) return no("out is a null pointer");
    if (n < 1 || T < 1) return no("n and T must be >= 1 (got " + S(n) + ", " + S(T) + ")");
    if (d.n_seg < 1) return no("the descriptor has no chain (n_seg = " + S(d.n_seg) + "): clearance needs the robot's kinematics");
    {
        DevChain ch;
        if (lower_chain(c, d, ch)) return no("the descriptor's chain is refused: " + c->err);
    }
    if (rb->n_sph < 1 || rb->n_sph > ILQR_CLR_MAX_SPH) return no("n_sph must be 1 .. " + S(ILQR_CLR_MAX_SPH) + " (got " + S(rb->n_sph) + ")");
    for (int i = 0; i < rb->n_sph; i++) {
        if (rb->sph_link[i] < -1 || rb->sph_link[i] >= d.n_seg)
            return no("sph_link[" + S(i) + "] = " + S(rb->sph_link[i]) + " is outside -1 .. " + S(d.n_seg - 1));
        if (i > 0 && rb->sph_link[i] < rb->sph_link[i - 1])
            return no("sph_link must be non-decreasing (sph_link[" + S(i) + "] = " + S(rb->sph_link[i]) + " follows " + S(rb->sph_link[i - 1]) + ")");
        if (!(std::isfinite(rb->sph_r[i]) && rb->sph_r[i] >= 0.0)) return no("sph_r[" + S(i) + "] must be finite and >= 0 (got " + std::to_string(rb->sph_r[i]) + ")");
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(rb->sph_c[i][a])) return no("sph_c[" + S(i) + "][" + S(a) + "] is not finite");
    }
    if (rb->n_planes < 0 || rb->n_planes > ILQR_CLR_MAX_PLANES) return no("n_planes must be 0 .. " + S(ILQR_CLR_MAX_PLANES) + " (got " + S(rb->n_planes) + ")");
    for (int l = 0; l < rb->n_planes; l++) {
        const double* nn = rb->plane_n[l];
        if (!(std::isfinite(nn[0]) && std::isfinite(nn[1]) && std::isfinite(nn[2]))) return no("plane_n[" + S(l) + "] is not finite");
        if (!(std::fabs(std::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]) - 1.0) <= 1e-9)) return no("plane_n[" + S(l) + "] is not a unit vector (| |n| - 1 | > 1e-9)");
        if (!std::isfinite(rb->plane_d[l])) return no("plane_d[" + S(l) + "] is not finite");
    }
    if (rb->n_self < 0 || rb->n_self > ILQR_CLR_MAX_SELF) return no("n_self must be 0 .. " + S(ILQR_CLR_MAX_SELF) + " (got " + S(rb->n_self) + ")");
    {
        bool anchor[ILQR_CLR_MAX_SPH] = {};
        int n_anchor = 0;
        for (int e = 0; e < rb->n_self; e++) {
            const int a = rb->self_pair[e][0], b = rb->self_pair[e][1];
            const std::string pe = "self_pair[" + S(e) + "] = (" + S(a) + ", " + S(b) + ")";
            if (a < 0 || a >= rb->n_sph || b < 0 || b >= rb->n_sph) return no(pe + " names a sphere outside 0 .. " + S(rb->n_sph - 1));
            if (a >= b) return no(pe + " must have a < b");
            if (rb->sph_link[a] == rb->sph_link[b]) return no(pe + ": both spheres are on link " + S(rb->sph_link[a]) + ", their distance is constant");
            bool moves = false;
            for (int s = rb->sph_link[a] + 1; s <= rb->sph_link[b]; s++) moves = moves || d.seg_joint[s] >= 0;
            if (!moves) return no(pe + ": no moving joint lies between link " + S(rb->sph_link[a]) + " and link " + S(rb->sph_link[b]) + ", their distance is constant");
            for (int f = 0; f < e; f++)
                if (rb->self_pair[f][0] == a && rb->self_pair[f][1] == b) return no(pe + " repeats self_pair[" + S(f) + "]");
            if (!anchor[a]) { anchor[a] = true; n_anchor++; }
        }
        if (n_anchor > ILQR_CLR_MAX_ANCHOR)
            return no("the self pairs have " + S(n_anchor) + " distinct first members (anchors); at most " + S(ILQR_CLR_MAX_ANCHOR) + " are supported");
    }
    if (w->n_obs < 0) return no("n_obs must be >= 0 (got " + S(w->n_obs) + ")");
    if (w->n_obs > CLR_MAX_OBS) return no("n_obs must be at most " + S(CLR_MAX_OBS) + " (got " + S(w->n_obs) + ")");
    if (rb->n_self > 0 && w->n_obs > CLR_MAX_OBS - ILQR_CLR_MAX_SPH)
        return no("n_obs must be at most " + S(CLR_MAX_OBS - ILQR_CLR_MAX_SPH) + " with self pairs (got " + S(w->n_obs) + ")");
    if (w->n_obs == 0 && rb->n_planes == 0 && rb->n_self == 0) return no("nothing to keep clear of: n_obs = 0 and n_planes = 0");
    if (w->n_obs > 0 && !w->obs) return no("obs is a null pointer with n_obs = " + S(w->n_obs));
    if (w->traj_per_set < 1 || n % w->traj_per_set != 0)
        return no("the number of trajectories (" + S(n) + ") is not a multiple of traj_per_set (" + S(w->traj_per_set) + ")");
    if (w->n_sets != n / w->traj_per_set)
        return no("n_sets must be n / traj_per_set = " + S(n / w->traj_per_set) + " (got " + S(w->n_sets) + ")");
    if (w->margin != w->margin) return no("margin is NaN");
    if (need_out && !out->clr && !out->clr_min && !out->clr_at && !out->n_below && !out->eligible && !out->stats) return no("every output is a null pointer");
    if (need_out && out->stats) {
        if (w->stats_group < 1) return no("stats needs stats_group >= 1 (got " + S(w->stats_group) + ")");
        if (n % w->stats_group != 0) return no("the number of trajectories (" + S(n) + ") is not a multiple of stats_group (" + S(w->stats_group) + ")");
    }
    if (!dev)
        for (size_t e = 0; e < (size_t)w->n_sets * (size_t)w->n_obs * 4; e++)
            if (!std::isfinite(w->obs[e]))
                return no("obs[" + S((long long)(e / ((size_t)w->n_obs * 4))) + "][" + S((long long)(e / 4 % (size_t)w->n_obs)) + "][" + S((long long)(e % 4)) + "] is not finite");
    return 0;
}

// The geometry as the kernels read it (checked by clr_check)
static void clr_fill_geom(const ilqr_problem_desc& d, const ilqr_clr_robot& rb, ClrGeom& g) {
    std::memset(&g, 0, sizeof(g));
    g.n_seg = d.n_seg; g.n_sph = rb.n_sph; g.n_planes = rb.n_planes;
    g.n_walk = rb.sph_link[rb.n_sph - 1] + 1;   // non-decreasing: the last sphere's link is the farthest
    std::memcpy(g.seg_joint, d.seg_joint, sizeof(int) * d.n_seg);
    std::memcpy(g.seg_xyz, d.seg_xyz, sizeof(double) * 3 * d.n_seg);
    std::memcpy(g.seg_R, d.seg_R, sizeof(double) * 9 * d.n_seg);
    std::memcpy(g.seg_axis, d.seg_axis, sizeof(double) * 3 * d.n_seg);
    std::memcpy(g.sph_link, rb.sph_link, sizeof(int) * rb.n_sph);
    std::memcpy(g.sph_c, rb.sph_c, sizeof(double) * 3 * rb.n_sph);
    std::memcpy(g.sph_r, rb.sph_r, sizeof(double) * rb.n_sph);
    std::memcpy(g.plane_n, rb.plane_n, sizeof(double) * 3 * rb.n_planes);
    std::memcpy(g.plane_d, rb.plane_d, sizeof(double) * rb.n_planes);
    // the self pairs: anchors in ascending sphere order, so that "slots ascending" is "anchors ascending"
    g.n_self = rb.n_self;
    for (int i = 0; i < ILQR_CLR_MAX_SPH; i++) g.self_slot[i] = -1;
    for (int i = 0; i < rb.n_sph; i++) {
        bool is_anchor = false;
        for (int e = 0; e < rb.n_self; e++) is_anchor = is_anchor || rb.self_pair[e][0] == i;
        if (!is_anchor) continue;
        const int t = g.n_anchor++;
        g.self_slot[i] = t;
        g.anc_sph[t] = i;
        g.anc_r[t] = rb.sph_r[i];
        for (int s = 0; s <= rb.sph_link[i]; s++) g.anc_first[t] += d.seg_joint[s] >= 0;   // joints are numbered in chain order (lower_chain)
    }
    for (int e = 0; e < rb.n_self; e++) g.self_mask[rb.self_pair[e][1]] |= 1 << g.self_slot[rb.self_pair[e][0]];
}

// p: the problem form (the plan where it lies); else X[n][T][n_x] in the natural layout of d
static int clr_run(ilqr_ctx* c, const char* fn_, ilqr_problem* p, const ilqr_problem_desc& d, int n, int T, const double* X, const ilqr_clr_robot* rb,
                   const ilqr_clr_world* w, const ilqr_clr_out* out_, bool dev) {
    const std::string fn = std::string(fn_) + (dev ? "_dev" : "");
    ilqr_dims ud;
    if (ilqr_dims_of(&d, &ud)) return fail(c, fn + ": unsupported system kind / nb_deriv");
    if (clr_check(c, fn, d, n, T, rb, w, out_, dev)) return 1;
    if (!p && !X) return fail(c, fn + ": X is a null pointer");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->clr) c->clr = new ClrState();
    ClrState& cs = *c->clr;
    ClrGeom g;
    clr_fill_geom(d, *rb, g);
    if (!cs.have || std::memcmp(&g, &cs.host, sizeof(g)) != 0) {   // kernels in flight may read the old one; the copy's source must outlive it
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (cs.geom.reserve(c, sizeof(ClrGeom))) return 1;
        cs.host = g;
        cs.have = false;
        HIPCHK(c, hipMemcpyAsync(cs.geom.ptr, &cs.host, sizeof(ClrGeom), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        cs.have = true;
    }
    const size_t nT = (size_t)n * (size_t)T;
    if (cs.ws.reserve(c, nT * 12)) return 1;
    ClrArgs a;
    std::memset(&a, 0, sizeof(a));
    a.geom = (const ClrGeom*)cs.geom.ptr;
    a.n_anchor = g.n_anchor;
    a.n = n; a.T = T; a.n_obs = w->n_obs; a.traj_per_set = w->traj_per_set;
    a.ws_clr = (double*)cs.ws.ptr;
    a.ws_code = (int*)(a.ws_clr + nT);
    for (int j = 0; j < DOF; j++) a.qrow[j] = j < d.dof ? (p ? p->map.x.dev[j] : j) : 0;
    a.obs = w->obs;
    ilqr_clr_out o = *out_;
    const int n_groups = out_->stats ? n / w->stats_group : 0;
    const size_t n_obs_all = (size_t)w->n_sets * (size_t)w->n_obs * 4, nX = p ? 0 : nT * (size_t)ud.n_x;
    if (!dev) {   // doubles: X | obs | clr | clr_min | stats; ints: clr_at | n_below | eligible
        const size_t nd = nX + n_obs_all + (out_->clr ? nT : 0) + (size_t)n + (size_t)n_groups * ILQR_CLR_STATS, ni = (size_t)5 * n;
        if (cs.io.reserve(c, nd * 8 + ni * 4)) return 1;
        double* q = (double*)cs.io.ptr;
        if (!p) { HIPCHK(c, hipMemcpyAsync(q, X, nX * 8, hipMemcpyHostToDevice, c->stream)); X = q; q += nX; }
        if (n_obs_all) { HIPCHK(c, hipMemcpyAsync(q, w->obs, n_obs_all * 8, hipMemcpyHostToDevice, c->stream)); a.obs = q; q += n_obs_all; }
        if (out_->clr) { o.clr = q; q += nT; }
        if (out_->clr_min) o.clr_min = q;
        q += n;
        if (out_->stats) o.stats = q;
        q += (size_t)n_groups * ILQR_CLR_STATS;
        int* qi = (int*)q;
        if (out_->clr_at) o.clr_at = qi;
        if (out_->n_below) o.n_below = qi + (size_t)3 * n;
        if (out_->eligible) o.eligible = qi + (size_t)4 * n;
    }
    {
        ProfScope ps(c, ILQR_PROF_OTHER);
        if (p) launch_clr_plan(p->bufs.X[0], p->bufs.X[1], p->bufs.cur, p->dims.n_x, p->Bp, a, c->stream);
        else launch_clr_traj(X, ud.n_x, a, c->stream);
    }
    const size_t stride_i = p ? 1 : (size_t)T, stride_k = p ? (size_t)n : 1;
    {
        ProfScope ps(c, ILQR_PROF_OTHER);
        launch_clr_fold(a, stride_i, stride_k, w->margin, o, c->stream);
    }
    if (out_->stats) {
        ProfScope ps(c, ILQR_PROF_OTHER);
        launch_clr_stats(o.clr_min ? o.clr_min : a.ws_clr, o.clr_min ? 1 : stride_i, n_groups, w->stats_group, w->margin, o.stats, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    prof_mark(c, -1);
    if (!dev) {
        if (out_->clr) HIPCHK(c, hipMemcpyAsync(out_->clr, o.clr, nT * 8, hipMemcpyDeviceToHost, c->stream));
        if (out_->clr_min) HIPCHK(c, hipMemcpyAsync(out_->clr_min, o.clr_min, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        if (out_->stats) HIPCHK(c, hipMemcpyAsync(out_->stats, o.stats, (size_t)n_groups * ILQR_CLR_STATS * 8, hipMemcpyDeviceToHost, c->stream));
        if (out_->clr_at) HIPCHK(c, hipMemcpyAsync(out_->clr_at, o.clr_at, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
        if (out_->n_below) HIPCHK(c, hipMemcpyAsync(out_->n_below, o.n_below, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        if (out_->eligible) HIPCHK(c, hipMemcpyAsync(out_->eligible, o.eligible, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

static int problem_clearance(ilqr_problem* p, const ilqr_clr_robot* rb, const ilqr_clr_world* w, const ilqr_clr_out* out, bool dev) {
    if (!p) return 1;
    if (!p->has_plan)
        return fail(p->ctx, std::string("ilqr_problem_clearance") + (dev ? "_dev" : "") + " needs a plan: run a solver since the problem's inputs last changed (ilqr_solve_recursive with nb_iter = 0 rolls out the controls as they are)");
    return clr_run(p->ctx, "ilqr_problem_clearance", p, p->desc, p->B, p->T, nullptr, rb, w, out, dev);
}
extern "C" int ilqr_problem_clearance(ilqr_problem* p, const ilqr_clr_robot* robot, const ilqr_clr_world* world, const ilqr_clr_out* out) {
    return problem_clearance(p, robot, world, out, false);
}
extern "C" int ilqr_problem_clearance_dev(ilqr_problem* p, const ilqr_clr_robot* robot, const ilqr_clr_world* world, const ilqr_clr_out* out) {
    return problem_clearance(p, robot, world, out, true);
}
extern "C" int ilqr_clearance_trajectories(ilqr_ctx* c, const ilqr_problem_desc* desc, int n, int T, const double* X, const ilqr_clr_robot* robot,
                                           const ilqr_clr_world* world, const ilqr_clr_out* out) {
    if (!c) return 1;
    if (!desc) return fail(c, "ilqr_clearance_trajectories: desc is a null pointer");
    return clr_run(c, "ilqr_clearance_trajectories", nullptr, *desc, n, T, X, robot, world, out, false);
}
extern "C" int ilqr_clearance_trajectories_dev(ilqr_ctx* c, const ilqr_problem_desc* desc, int n, int T, const double* X, const ilqr_clr_robot* robot,
                                               const ilqr_clr_world* world, const ilqr_clr_out* out) {
    if (!c) return 1;
    if (!desc) return fail(c, "ilqr_clearance_trajectories_dev: desc is a null pointer");
    return clr_run(c, "ilqr_clearance_trajectories", nullptr, *desc, n, T, X, robot, world, out, true);
}

// ------------------------------------------------------------------------------------------------ obstacle terms
// include/ilqr_hip.h "obstacle terms".  The setter copies everything it is given into device memory of the problem (the geometry block of the
// clearance kernels, the obstacle sets, and the slots k_obs_derivs fills before every sweep); from then on plan_input routes the problem to the
// generic kernels, whose OBS forms read the terms.

static int set_obstacles(ilqr_problem* p, const ilqr_clr_robot* rb, const ilqr_clr_world* w, double weight, bool dev) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    const std::string fn = std::string("ilqr_problem_set_obstacles") + (dev ? "_dev" : "");
    if (!rb) {   // remove the terms: the problem is planned as before
        p->has_obs = false;
        p->has_gains = p->has_plan = false;
        return 0;
    }
    if (clr_check(c, fn, p->desc, p->B, p->T, rb, w, nullptr, dev, false)) return 1;
    if (std::isinf(w->margin)) return fail(c, fn + ": margin is infinite");
    if (!(std::isfinite(weight) && weight >= 0.0)) return fail(c, fn + ": the weight must be finite and >= 0 (got " + std::to_string(weight) + ")");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // kernels in flight may read the previous terms
    p->has_obs = false;
    p->has_gains = p->has_plan = false;
    ClrGeom g;
    clr_fill_geom(p->desc, *rb, g);
    if (!p->obs.geom) HIPCHK(c, hipMalloc((void**)&p->obs.geom, sizeof(ClrGeom)));
    if (!p->obs.obd) HIPCHK(c, hipMalloc((void**)&p->obs.obd, sizeof(double) * (size_t)p->T * OBS_W * (size_t)p->Bp));
    const size_t bytes = sizeof(double) * (size_t)w->n_sets * (size_t)w->n_obs * 4;
    if (bytes > p->obs_sets_bytes) {
        if (p->obs.obs) HIPCHK(c, hipFree((void*)p->obs.obs));
        p->obs.obs = nullptr;
        p->obs_sets_bytes = 0;
        HIPCHK(c, hipMalloc((void**)&p->obs.obs, bytes));
        p->obs_sets_bytes = bytes;
    }
    HIPCHK(c, hipMemcpyAsync((void*)p->obs.geom, &g, sizeof(ClrGeom), hipMemcpyHostToDevice, c->stream));
    if (bytes) HIPCHK(c, hipMemcpyAsync((void*)p->obs.obs, w->obs, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // g is on this stack; the caller's arrays may go away
    p->obs.n_obs = w->n_obs; p->obs.traj_per_set = w->traj_per_set; p->obs.margin = w->margin; p->obs.weight = weight;
    p->obs.n_anchor = g.n_anchor;
    p->has_obs = true;
    return 0;
}
extern "C" int ilqr_problem_set_obstacles(ilqr_problem* p, const ilqr_clr_robot* robot, const ilqr_clr_world* world, double weight) {
    return set_obstacles(p, robot, world, weight, false);
}
extern "C" int ilqr_problem_set_obstacles_dev(ilqr_problem* p, const ilqr_clr_robot* robot, const ilqr_clr_world* world, double weight) {
    return set_obstacles(p, robot, world, weight, true);
}

static int obstacle_terms(ilqr_problem* p, double* cost, double* lx, double* lxx, bool dev) {
    if (!p) return 1;
    ilqr_ctx* c = p->ctx;
    const std::string fn = std::string("ilqr_problem_obstacle_terms") + (dev ? "_dev" : "");
    if (!p->has_obs) return fail(c, fn + ": the problem has no obstacle terms (ilqr_problem_set_obstacles)");
    if (!p->has_plan)
        return fail(c, fn + " needs a plan: run a solver since the problem's inputs last changed (ilqr_solve_recursive with nb_iter = 0 rolls out the controls as they are)");
    if (!cost && !lx && !lxx) return fail(c, fn + ": every output is a null pointer");
    HIPCHK(c, hipSetDevice(c->device));
    const int dof = p->desc.dof;
    const size_t nT = (size_t)p->B * (size_t)p->T, n_lx = nT * dof, n_lxx = n_lx * dof;
    double *dc = cost, *dl = lx, *dm = lxx;
    if (!dev) {
        if (p->staging.reserve(c, nT + n_lx + n_lxx)) return 1;
        dc = cost ? p->staging.ptr : nullptr;
        dl = lx ? p->staging.ptr + nT : nullptr;
        dm = lxx ? p->staging.ptr + nT + n_lx : nullptr;
    }
    {
        ProfScope ps(c, ILQR_PROF_OTHER);
        if (p->obs.n_anchor) launch_obs_derivs_self(p->bufs, p->obs, p->B, p->T, p->dims.n_x, 1, c->stream);
        else launch_obs_derivs(p->bufs, p->obs, p->B, p->T, p->dims.n_x, 1, c->stream);
    }
    {
        ProfScope ps(c, ILQR_PROF_OTHER);
        launch_obs_query(p->obs, p->B, p->Bp, p->T, dof, dc, dl, dm, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    prof_mark(c, -1);
    if (!dev) {
        if (cost) HIPCHK(c, hipMemcpyAsync(cost, dc, nT * 8, hipMemcpyDeviceToHost, c->stream));
        if (lx) HIPCHK(c, hipMemcpyAsync(lx, dl, n_lx * 8, hipMemcpyDeviceToHost, c->stream));
        if (lxx) HIPCHK(c, hipMemcpyAsync(lxx, dm, n_lxx * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}
extern "C" int ilqr_problem_obstacle_terms(ilqr_problem* p, double* cost, double* lx, double* lxx) { return obstacle_terms(p, cost, lx, lxx, false); }
extern "C" int ilqr_problem_obstacle_terms_dev(ilqr_problem* p, double* cost, double* lx, double* lxx) { return obstacle_terms(p, cost, lx, lxx, true); }

// ------------------------------------------------------------------------------------------------ stand-alone FK

extern "C" int ilqr_fk_batch(ilqr_ctx* c, const ilqr_problem_desc* d, int n, const double* q, double* pos, double* quat, double* jac) {
    if (!c) return 1;
    if (!d || n <= 0 || !q) return fail(c, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    DevDesc h;
    std::memset(&h, 0, sizeof(h));
    if (lower_chain(c, *d, h.chain)) return 1;
    const int dof = d->dof;  // a chain of fewer than 7 joints runs as 7 with the inert joints at q = 0 (ilqr_dofmap.hpp)
    std::vector<double> qw, jw;
    if (dof != DOF) {
        qw.assign((size_t)n * DOF, 0.0);
        for (int i = 0; i < n; i++) std::memcpy(&qw[(size_t)i * DOF], q + (size_t)i * dof, sizeof(double) * dof);
        q = qw.data();
        if (jac) jw.resize((size_t)n * 6 * DOF);
    }
    double* jac_out = jac;
    if (jac && dof != DOF) jac = jw.data();
    DevDesc* dd = nullptr;
    double *dq = nullptr, *dp = nullptr, *dqt = nullptr, *dj = nullptr;
    int rc = 0;
    auto cleanup = [&]() { (void)hipFree(dd); (void)hipFree(dq); (void)hipFree(dp); (void)hipFree(dqt); (void)hipFree(dj); };
#define FKCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { cleanup(); return fail(c, std::string(#call) + ": " + hipGetErrorString(e_)); } } while (0)
    FKCHK(hipMalloc((void**)&dd, sizeof(DevDesc)));
    FKCHK(hipMalloc((void**)&dq, sizeof(double) * n * DOF));
    if (pos) FKCHK(hipMalloc((void**)&dp, sizeof(double) * n * 3));
    if (quat) FKCHK(hipMalloc((void**)&dqt, sizeof(double) * n * 4));
    if (jac) FKCHK(hipMalloc((void**)&dj, sizeof(double) * n * 6 * DOF));
    FKCHK(hipMemcpyAsync(dd, &h, sizeof(DevDesc), hipMemcpyHostToDevice, c->stream));
    FKCHK(hipMemcpyAsync(dq, q, sizeof(double) * n * DOF, hipMemcpyHostToDevice, c->stream));
    launch_fk_batch(dd, n, dq, dp, dqt, dj, c->stream);
    FKCHK(hipGetLastError());
    if (pos) FKCHK(hipMemcpyAsync(pos, dp, sizeof(double) * n * 3, hipMemcpyDeviceToHost, c->stream));
    if (quat) FKCHK(hipMemcpyAsync(quat, dqt, sizeof(double) * n * 4, hipMemcpyDeviceToHost, c->stream));
    if (jac) FKCHK(hipMemcpyAsync(jac, dj, sizeof(double) * n * 6 * DOF, hipMemcpyDeviceToHost, c->stream));
    FKCHK(hipStreamSynchronize(c->stream));
#undef FKCHK
    cleanup();
    if (jac && dof != DOF)
        for (size_t r = 0; r < (size_t)n * 6; r++) std::memcpy(jac_out + r * dof, &jw[r * DOF], sizeof(double) * dof);
    return rc;
}

// the kernels that join instances (adopt, spread, select, get_at) and their launchers: this is the one translation unit that defines them
#define ILQR_MULTISTART_KERNELS_TU
#include "ilqr_multistart_kernels.hpp"

// the clearance kernels (per state, fold, stats) and their launchers: likewise
#define ILQR_CLEARANCE_KERNELS_TU
#include "ilqr_clearance_kernels.hpp"

// the lane-per-item kernels of the obstacle terms' cooperative path (k_stage_dense, k_obs_ls, k_obs_ls_sum) and their launchers: likewise
#include "ilqr_obstacle_coop_kernels.hpp"
