// ilqr_capi_ctx.cpp -- C ABI (include/ilqr_hip.h): version, descriptor defaults and dimensions, the context and its setters, profiling.
#include "ilqr_capi_internal.hpp"

using namespace ilqr_capi;

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

namespace ilqr_capi {
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
void prof_mark(ilqr_ctx* c, int which) {  // which < 0: end mark (closes the previous interval, charges nothing itself)
    if (!c->profile) return;
    hipEvent_t e = ev_get(c);
    (void)hipEventRecord(e, c->stream);
    c->pending.push_back({e, nullptr, which});
    if (which < 0 && c->pending.size() > 4096) prof_collect(c);  // synchronises; only with profiling on and only every few hundred solves
}


static void prof_hook_fn(void* c, int which) { prof_mark((ilqr_ctx*)c, which); }
ProfHook prof_hook(ilqr_ctx* c) {
    ProfHook h;
    if (c->profile) { h.mark = prof_hook_fn; h.ctx = c; }
    return h;
}
}  // namespace ilqr_capi

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
