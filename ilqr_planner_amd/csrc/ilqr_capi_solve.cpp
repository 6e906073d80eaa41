// ilqr_capi_solve.cpp -- C ABI (include/ilqr_hip.h): the solvers.  The per-iteration launch sequence
//   init rollout -> nb_iter x { backward sweep, forward line search }
// mirrors ILQRRecursive::solve / AL_ILQR::solve (reference src/solver/ILQRRecursive.cpp:21-181, src/solver/AL-ILQR.cpp:50-232); the two batch
// solvers; the gains about a held plan.
#include "ilqr_capi_internal.hpp"

using namespace ilqr_capi;

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
    launch_obs_derivs_any(bf, p->obs, B, p->T, p->dims.n_x, 0, st);
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
        else launch_init_obs(kind, nd, al, bf, hv[h].B, hv[h].st, penalty0, p->has_obs ? &p->obs : nullptr);
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
                    case Forward::Generic: launch_forward_generic_obs(kind, nd, al, bf, B, st, fi, p->has_obs ? &p->obs : nullptr); break;
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
