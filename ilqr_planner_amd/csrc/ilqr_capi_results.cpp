// ilqr_capi_results.cpp -- C ABI (include/ilqr_hip.h): layout conversion on the way out (the getters, the trace, f(X)), warm start and tracking.
#include "ilqr_capi_internal.hpp"

using namespace ilqr_capi;

// ------------------------------------------------------------------------------------------------ results

enum { GET_PLAIN, GET_CUR, GET_SCALED };
// SoA [rows][Bp] -> natural [B][rows]; with a map m (GET_CUR only): [outer][m->n_dev][Bp] -> natural [B][outer][m->n_user], rows = outer * m->n_user
static int download(ilqr_problem* p, int mode, const double* s0, const double* s1, double* dst, bool dst_is_dev, int rows, const IndexMap* m = nullptr,
                    int outer = 0) {
    ilqr_ctx* c = p->ctx;
    if (!dst) return fail(c, "null output pointer");
    const size_t n = (size_t)p->B * rows;
    double* ddst = dst;
    Staging stg{c};
    if (!dst_is_dev && stg.lay(p->staging, [&](Staging& s) { ddst = s.take_out(dst, n); })) return 1;
    if (m) launch_from_soa_cur_map(s0, s1, p->bufs.cur, ddst, p->B, p->Bp, outer, *m, c->stream);
    else if (mode == GET_CUR) launch_from_soa_cur(s0, s1, p->bufs.cur, ddst, p->B, p->Bp, rows, c->stream);
    else if (mode == GET_SCALED) launch_from_soa_scaled(s0, p->bufs.alpha, p->bufs.iters, ddst, p->B, p->Bp, rows, c->stream);
    else launch_from_soa(s0, ddst, p->B, p->Bp, rows, c->stream);
    HIPCHK(c, hipGetLastError());
    return dst_is_dev ? 0 : stg.fetch();
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
    double* s = nullptr;
    Staging stg{c};
    if (stg.lay(p->staging, [&](Staging& g) { s = g.take_out(dst, n); })) return 1;
    if (p->mapped) launch_get_gains_map(p->bufs.KD, p->bufs.kd_sym, p->bufs.alpha, p->bufs.iters, K ? s : nullptr, K ? nullptr : s, p->B, p->Bp, T1, p->map, c->stream);
    else launch_get_gains(p->bufs.KD, p->bufs.kd_sym, p->bufs.alpha, p->bufs.iters, K ? s : nullptr, K ? nullptr : s, p->B, p->Bp, T1, nu, nx, c->stream);
    HIPCHK(c, hipGetLastError());
    return stg.fetch();
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
    const bool narrow = p->udims.n_f != p->dims.n_f;  // f(x) = x of a joint-space system of fewer than 7 joints: the state map
    std::vector<double> wide(narrow ? n : 0);
    double* s = nullptr;
    Staging stg{c};
    if (stg.lay(p->staging, [&](Staging& g) { s = g.take_out(narrow ? wide.data() : fX, n); })) return 1;
    {
        ProfScope ps(c, ILQR_PROF_OTHER);
        launch_fx_all(p->desc.kind, p->desc.nb_deriv, p->bufs, p->B, p->T, s, c->stream);
    }
    prof_mark(c, -1);
    HIPCHK(c, hipGetLastError());
    if (stg.fetch()) return 1;
    if (narrow) {
        const IndexMap& mx = p->map.x;
        for (size_t r = 0; r < (size_t)p->B * p->T; r++)
            for (int i = 0; i < mx.n_user; i++) fX[r * mx.n_user + i] = wide[r * mx.n_dev + mx.dev[i]];
    }
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
    Staging stg{c};
    if (!dev && stg.lay(p->staging, [&](Staging& s) { xs = s.take_in(x_meas, nxb); us = s.take_out(u_out, nub); })) return 1;
    if (p->mapped) launch_track_map(p->bufs, xs, k, with_ff, us, p->B, p->map, c->stream);
    else launch_track(p->bufs, xs, k, with_ff, us, p->B, p->dims.n_x, p->dims.n_u, c->stream);
    HIPCHK(c, hipGetLastError());
    return dev ? 0 : stg.fetch();
}
extern "C" int ilqr_problem_track(ilqr_problem* p, int k, const double* x_meas, int with_feedforward, double* u_out) {
    return track(p, k, x_meas, with_feedforward, u_out, false);
}
extern "C" int ilqr_problem_track_dev(ilqr_problem* p, int k, const double* x_meas, int with_feedforward, double* u_out) {
    return track(p, k, x_meas, with_feedforward, u_out, true);
}
