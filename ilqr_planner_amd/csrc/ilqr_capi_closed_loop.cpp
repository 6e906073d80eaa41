// ilqr_capi_closed_loop.cpp -- C ABI (include/ilqr_hip.h): the closed loop of the tracking law and its covariance, fourteen entry points.
#include "ilqr_capi_internal.hpp"

using namespace ilqr_capi;

// ------------------------------------------------------------------------------------------------ closed loop
// Closed loop of the tracking law on the last plan (ilqr_closed_loop.hpp): n_samples executions per instance.  Which kernel runs is decided by
// plan_closed_loop; chains of fewer than 7 joints take the generic kernel's mapped variant.  Each of the six entry points fills a ClRequest, and
// closed_loop does its jobs in turn: cl_check (every refusal), cl_bind (the memory the kernels see every array in), cl_launch and, for host
// pointers, Staging::fetch.
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

struct ClBound {  // what the kernels see
    ClArgs a;
    double* stats = nullptr;  // the device side of stats
    ilqr_cl_report dr = {};   // ... and of the four report outputs
    ilqr_cl_con dc = {};      // ... and of the four outputs of the constraints
};

// Per array: the caller's device pointer, a slice of staging (host pointers), or a workspace of the problem (what the caller does not ask for
// but a kernel reads).  rq has passed cl_check.
static int cl_bind(ilqr_problem* p, const ClRequest& rq, const ClosedLoopPlan& pl, Staging& stg, ClBound& b) {
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
        if (p->cl_kpx.reserve_doubles(c, (size_t)(p->hdesc.steps.n > 0 ? p->hdesc.steps.n : 1) * (p->dims.n_x + p->dims.n_u) * n)) return 1;
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
            if (p->cl_cost.reserve_doubles(c, n)) return 1;
            a.cost = p->cl_cost.doubles();
        }
        if (rq.report) {  // kp_err | lim_cost where the caller asks only for their reductions
            const size_t ws_ke = rp.kp_err ? 0 : n_ke, ws_lc = rp.lim_cost ? 0 : n_lc;
            if (p->cl_rep.reserve_doubles(c, ws_ke + ws_lc)) return 1;
            if (!rp.kp_err) b.dr.kp_err = p->cl_rep.doubles();
            if (!rp.lim_cost) b.dr.lim_cost = p->cl_rep.doubles() + ws_ke;
        }
        if (rq.con) {  // con_max | con_steps likewise
            const size_t ws_cm = oc.con_max ? 0 : n_cm, ws_cs = oc.con_steps ? 0 : n_cs;
            if (p->cl_con_ws.reserve_doubles(c, ws_cm + ws_cs)) return 1;
            if (!oc.con_max) b.dc.con_max = p->cl_con_ws.doubles();
            if (!oc.con_steps) b.dc.con_steps = p->cl_con_ws.doubles() + ws_cm;
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
    }
    if (rq.report) { a.kpx = pl.coop ? nullptr : p->cl_kpx.doubles(); a.lim_cost = want_lc ? b.dr.lim_cost : nullptr; }
    if (rq.con) { a.con_tol = rq.con_tol; a.con_max = want_cm ? b.dc.con_max : nullptr; a.con_steps = want_cs ? b.dc.con_steps : nullptr; }
    return 0;
}

static void cl_launch(ilqr_problem* p, const ClRequest& rq, const ClosedLoopPlan& pl, const ClBound& b) {
    const int kind = p->desc.kind, nd = p->desc.nb_deriv, B = p->B, S = rq.S, n_kp = p->hdesc.steps.kp[p->hdesc.steps.n];
    hipStream_t st = p->ctx->stream;
    if (pl.coop) launch_closed_loop_coop(kind, nd, p->bufs, b.a, B, pl, p->cl_kpx.doubles(), st);
    else launch_closed_loop(kind, nd, p->bufs, b.a, B, p->mapped ? &p->map : nullptr, st);
    if (rq.stats) launch_closed_loop_stats(b.a.cost, B, S, b.stats, st);
    if (!rq.report) return;
    const ilqr_cl_report rp = rq.rep();
    const ilqr_cl_con oc = rq.cons();
    if (rp.kp_err || rp.kp_stats || rp.outcome || oc.outcome_con) launch_closed_loop_kp_err(kind, nd, p->bufs, B, S, n_kp, p->cl_kpx.doubles(), b.dr.kp_err, st);
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
    Staging stg{c};
    if (rq.dev ? cl_bind(p, rq, pl, stg, b) : stg.lay(p->staging, [&](Staging& s) { return cl_bind(p, rq, pl, s, b); })) return 1;
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
// cr: ilqr_problem_closed_loop_cov_clr -- `out_` may be null; the covariance kernels run as they are, with Sigma in a buffer of the context where
// the caller does not ask for it, and k_cov_clr / k_cov_clr_fold (ilqr_cov_clearance.hpp) read the clearance pairs off it.
struct CovClrRequest {
    const ilqr_clr_robot* robot;
    const ilqr_clr_world* world;
    double z_tol;
    const ilqr_cl_cov_clr* clr;
};
static int closed_loop_cov(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out_, bool dev, bool with_con = false,
                           const ilqr_cl_cov_con* con = nullptr, const CovClrRequest* cr = nullptr) {
    if (!p) return 1;
    const ilqr_cl_cov none = {};
    const ilqr_cl_cov* out = ((with_con || cr) && !out_) ? &none : out_;
    const ilqr_cl_cov_clr ok = (cr && cr->clr) ? *cr->clr : ilqr_cl_cov_clr{};
    const bool want_clr = ok.clr_var || ok.clr_z || ok.clr_z_min || ok.clr_z_at || ok.eligible;
    const std::string clr_fn = std::string("ilqr_problem_closed_loop_cov_clr") + (dev ? "_dev" : "");
    const ilqr_cl_cov_con oc = (with_con && con) ? *con : ilqr_cl_cov_con{};
    ilqr_ctx* c = p->ctx;
    const int T = p->T, nxu = p->udims.n_x, nuu = p->udims.n_u, B = p->B, n_kp = p->hdesc.steps.kp[p->hdesc.steps.n];
    for (int i = 0; i < nxu; i++)
        for (const double* sg : {sigma_w, sigma_x0})
            if (sg && (!(sg[i] >= 0) || !std::isfinite(sg[i]))) return fail(c, "closed loop: every sigma_w and sigma_x0 must be finite and >= 0");
    const bool no_out = !out || (!out->Sigma && !out->kp_Sigma && !out->kp_var && !out->u_var && !out->lim_z);
    if (!with_con && !cr && no_out) return fail(c, "closed loop cov: every output is a null pointer");
    const size_t nn = (size_t)nxu * nxu, n_S = (size_t)B * T * nn, n_kS = (size_t)B * n_kp * nn;
    if (const char* why = cl_cov_size_refusal(B, T, n_kp, nxu, out->Sigma != nullptr || want_clr, out->kp_Sigma != nullptr)) return fail(c, why);
    if (!p->has_gains)   // (behind the bounds on the call itself: those do not depend on the state of the problem)
        return fail(c, "closed loop needs the gains of a Riccati solve (ilqr_solve_recursive or ilqr_solve_al with nb_iter >= 1) or of ilqr_problem_gains since the problem's inputs last changed");
    if (with_con) {
        if (p->bufs.m <= 0) return fail(c, "closed loop cov con: no constraints set");
        if (no_out && !oc.con_var && !oc.con_z) return fail(c, "closed loop cov con: con and out both ask for nothing");
    }
    if (cr) {
        if (clr_check_world(c, clr_fn, p->desc, B, T, cr->robot, cr->world, dev)) return 1;
        if (std::isnan(cr->z_tol)) return fail(c, clr_fn + ": z_tol is NaN");
        if (no_out && !want_clr) return fail(c, clr_fn + ": clr and out both ask for nothing");
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
    CovClrArgs ca;
    std::memset(&ca, 0, sizeof(ca));
    ilqr_cl_cov_clr dk = ok;   // the device side of the five outputs
    const size_t nT = (size_t)B * (size_t)T;
    const size_t n_obs_all = want_clr ? (size_t)cr->world->n_sets * (size_t)cr->world->n_obs * 4 : 0;
    if (want_clr) ca.obs = cr->world->obs;
    auto bind = [&](Staging& stg) {  // the staging slices of a host-pointer call (Staging::lay: first the sizing walk, then the real one)
        if (out->Sigma || want_clr) a.Sigma = stg.take_out(out->Sigma, n_S);   // k_cov_clr reads it there, asked for or not
        if (n_obs_all) ca.obs = stg.take_in(cr->world->obs, n_obs_all);
        if (ok.clr_var) dk.clr_var = stg.take_out(ok.clr_var, nT);
        if (ok.clr_z) dk.clr_z = stg.take_out(ok.clr_z, nT);
        if (ok.clr_z_min) dk.clr_z_min = stg.take_out(ok.clr_z_min, (size_t)B);
        if (ok.clr_z_at) dk.clr_z_at = stg.take_out(ok.clr_z_at, (size_t)3 * B);
        if (ok.eligible) dk.eligible = stg.take_out(ok.eligible, (size_t)B);
        a.kp_Sigma = want_kS ? stg.take_out(out->kp_Sigma, n_kS) : nullptr;
        if (out->kp_var) kp_var = stg.take_out(out->kp_var, n_kv);
        if (out->u_var) a.u_var = stg.take_out(out->u_var, n_uv);
        if (out->lim_z) a.lim_z = stg.take_out(out->lim_z, (size_t)B);
        if (oc.con_var) a.con_var = stg.take_out(oc.con_var, n_cv);
        if (oc.con_z) a.con_z = stg.take_out(oc.con_z, (size_t)B);
    };
    Staging stg{c};
    if (!dev) {
        if (stg.lay(p->staging, bind)) return 1;
    } else {
        if (want_kS && !out->kp_Sigma) {
            if (p->cl_cov_kps.reserve_doubles(c, n_kS)) return 1;
            a.kp_Sigma = p->cl_cov_kps.doubles();
        }
        if (want_clr && !out->Sigma) {
            DevScratch& sg = clr_cov_scratch(c, 0);
            if (sg.reserve_doubles(c, n_S)) return 1;
            a.Sigma = sg.doubles();
        }
    }
    if (want_clr) {
        if (clr_bind_geom(c, p->desc, *cr->robot, &ca.geom, &ca.n_anchor)) return 1;
        DevScratch& ws = clr_cov_scratch(c, 1);
        if (ws.reserve(c, nT * 20)) return 1;
        ca.Sigma = a.Sigma;
        ca.n = B; ca.T = T; ca.n_obs = cr->world->n_obs; ca.traj_per_set = cr->world->traj_per_set; ca.n_x = nxu; ca.dof = p->desc.dof;
        ca.margin = cr->world->margin;
        ca.ws_z = ws.doubles();
        ca.ws_var = ca.ws_z + nT;
        ca.ws_code = (int*)(ca.ws_var + nT);
        for (int j = 0; j < DOF; j++) ca.qrow[j] = j < p->desc.dof ? p->map.x.dev[j] : 0;
    }
    if (!want_kS) a.kp_Sigma = nullptr;
    if (!pl.rows) {
        if (p->cl_cov_ws.reserve_doubles(c, (size_t)cl_cov_ws_entries(p->desc.kind, p->desc.nb_deriv) * p->Bp)) return 1;
        a.ws = p->cl_cov_ws.doubles();
    }
    const int kind = p->desc.kind, nd = p->desc.nb_deriv;
    if (pl.rows) launch_closed_loop_cov_rows(kind, nd, p->bufs, a, B, c->stream);
    else launch_closed_loop_cov(kind, nd, p->bufs, a, B, p->mapped ? &p->map : nullptr, c->stream);
    if (out->kp_var) launch_closed_loop_cov_kp(kind, nd, p->bufs, B, n_kp, p->mapped ? p->map.dof : DOF, a.kp_Sigma, kp_var, c->stream);
    if (want_clr) {
        {
            ProfScope ps(c, ILQR_PROF_OTHER);
            launch_cov_clr(p->bufs.X[0], p->bufs.X[1], p->bufs.cur, p->dims.n_x, p->Bp, ca, c->stream);
        }
        {
            ProfScope ps(c, ILQR_PROF_OTHER);
            launch_cov_clr_fold(ca, cr->z_tol, dk, c->stream);
        }
        prof_mark(c, -1);
    }
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

extern "C" int ilqr_problem_closed_loop_cov_clr(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out,
                                                const ilqr_clr_robot* robot, const ilqr_clr_world* world, double z_tol, const ilqr_cl_cov_clr* clr) {
    const CovClrRequest cr{robot, world, z_tol, clr};
    return closed_loop_cov(p, sigma_w, sigma_x0, out, false, false, nullptr, &cr);
}
extern "C" int ilqr_problem_closed_loop_cov_clr_dev(ilqr_problem* p, const double* sigma_w, const double* sigma_x0, const ilqr_cl_cov* out,
                                                    const ilqr_clr_robot* robot, const ilqr_clr_world* world, double z_tol, const ilqr_cl_cov_clr* clr) {
    const CovClrRequest cr{robot, world, z_tol, clr};
    return closed_loop_cov(p, sigma_w, sigma_x0, out, true, false, nullptr, &cr);
}
