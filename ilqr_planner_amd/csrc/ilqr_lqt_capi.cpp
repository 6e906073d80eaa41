// ilqr_lqt_capi.cpp -- the ilqr_lqt_* entry points of include/ilqr_hip.h: batched linear-quadratic tracking (solver::LQT, reference
// src/solver/lqt.cpp).  Buffer ownership, argument checks and the launch order; the kernels are in ilqr_lqt.hip.  Kept apart from
// the units of ilqr_capi_*.cpp, which reference none of these symbols: a handle is freed with its context through ilqr_ctx::cleanups.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/ilqr_hip.h"
#include "ilqr_ctx.hpp"
#include "ilqr_lqt.hpp"

using namespace ilqr;

struct ilqr_lqt {
    ilqr_ctx* ctx = nullptr;
    LqtDev dv;
    void* mem = nullptr;         // one allocation for every device buffer
    double* staging = nullptr;   // [B][n_x + n_u]: host x / u of ilqr_lqt_command
    bool has_targets = false, dp_done = false, linal_done = false;
};

static const char* kDpFirst = "solveDP() first";                    // lqt.cpp:108
static const char* kLinalFirst = "solveLinal() or solveQP() first";  // lqt.cpp:97,124

static void lqt_destroy_cb(void* h) { ilqr_lqt_destroy(static_cast<ilqr_lqt*>(h)); }

extern "C" int ilqr_lqt_create(ilqr_ctx* c, int n_x, int n_u, int N, int batch, const double* A, const double* Bm, double r, const double* Qs,
                               int qs_per_instance, ilqr_lqt** out) {
    if (!c || !out) return 1;
    *out = nullptr;
    if (n_x < 1 || n_x > ILQR_LQT_MAX_NX)
        return fail(c, "ilqr_lqt_create: n_x must be in 1.." + std::to_string(ILQR_LQT_MAX_NX) + " (got " + std::to_string(n_x) + ")");
    if (n_u < 1 || n_u > ILQR_LQT_MAX_NU)
        return fail(c, "ilqr_lqt_create: n_u must be in 1.." + std::to_string(ILQR_LQT_MAX_NU) + " (got " + std::to_string(n_u) + ")");
    if (N < 1) return fail(c, "ilqr_lqt_create: N must be >= 1 (got " + std::to_string(N) + ")");
    if (batch < 1) return fail(c, "ilqr_lqt_create: batch must be >= 1 (got " + std::to_string(batch) + ")");
    if (!A || !Bm || !Qs) return fail(c, "ilqr_lqt_create: null A, B or Qs");
    HIPCHK(c, hipSetDevice(c->device));
    const int n = n_x, m = n_u, B = batch, chains = qs_per_instance ? B : 1;
    const size_t nn = (size_t)n * n, mn = (size_t)m * n, cN = (size_t)chains * N;
    const size_t sizes[] = {nn,                      // A
                            mn,                      // B
                            cN * nn,                 // Q
                            (size_t)B * N * n,       // mu
                            cN * nn,                 // P
                            cN * mn,                 // L
                            cN * mn,                 // H
                            chains == 1 ? N * nn : 0,  // W
                            (size_t)B * N * n,       // d
                            (size_t)B * (N - 1) * m, // U
                            (size_t)B * N * n,       // X
                            (size_t)B * (n + m),     // staging
                            64};                     // dump
    size_t total = 0;
    for (size_t s : sizes) total += (s + 1) & ~(size_t)1;  // 16-byte aligned starts
    auto* h = new ilqr_lqt();
    h->ctx = c;
    if (hipMalloc(&h->mem, total * sizeof(double)) != hipSuccess) {
        delete h;
        return fail(c, "ilqr_lqt_create: out of device memory (" + std::to_string(total * sizeof(double)) + " bytes)");
    }
    double* ptr[13];
    double* p = static_cast<double*>(h->mem);
    for (int i = 0; i < 13; i++) {
        ptr[i] = p;
        p += (sizes[i] + 1) & ~(size_t)1;
    }
    LqtDev& d = h->dv;
    d.n = n; d.m = m; d.N = N; d.B = B; d.chains = chains; d.r = r;
    d.A = ptr[0]; d.Bm = ptr[1]; d.Q = ptr[2]; d.mu = ptr[3]; d.P = ptr[4]; d.L = ptr[5]; d.H = ptr[6];
    d.W = ptr[7]; d.d = ptr[8]; d.U = ptr[9]; d.X = ptr[10];
    h->staging = ptr[11];
    d.dump = ptr[12];
    // The kernels take P to be symmetric; Q enters as (Q + Q') / 2, which is Q itself, bit for bit, for a symmetric precision.
    std::vector<double> q(Qs, Qs + cN * nn);
    for (size_t k = 0; k < cN; k++) {
        double* Qk = q.data() + k * nn;
        for (int i = 0; i < n; i++)
            for (int j = i + 1; j < n; j++) Qk[i * n + j] = Qk[j * n + i] = 0.5 * (Qk[i * n + j] + Qk[j * n + i]);
    }
    int rc = 0;
    if (hipMemcpyAsync(const_cast<double*>(d.A), A, nn * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(const_cast<double*>(d.Bm), Bm, mn * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(const_cast<double*>(d.Q), q.data(), q.size() * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        rc = fail(c, "ilqr_lqt_create: upload failed");
    if (rc) {
        (void)hipFree(h->mem);
        delete h;
        return rc;
    }
    c->cleanups.push_back({lqt_destroy_cb, h});
    *out = h;
    return 0;
}

extern "C" void ilqr_lqt_destroy(ilqr_lqt* h) {
    if (!h) return;
    ilqr_ctx* c = h->ctx;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(h->mem);
    auto& v = c->cleanups;
    v.erase(std::remove_if(v.begin(), v.end(), [h](const ilqr_ctx::Cleanup& e) { return e.handle == h; }), v.end());
    delete h;
}

static int set_targets(ilqr_lqt* h, const double* mu, bool dev) {
    if (!h) return 1;
    ilqr_ctx* c = h->ctx;
    if (!mu) return fail(c, "ilqr_lqt_set_targets: null mu");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)h->dv.B * h->dv.N * h->dv.n * sizeof(double);
    HIPCHK(c, hipMemcpyAsync(const_cast<double*>(h->dv.mu), mu, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    if (!dev) HIPCHK(c, hipStreamSynchronize(c->stream));
    h->has_targets = true;
    h->dp_done = h->linal_done = false;
    return 0;
}
extern "C" int ilqr_lqt_set_targets(ilqr_lqt* h, const double* mu) { return set_targets(h, mu, false); }
extern "C" int ilqr_lqt_set_targets_dev(ilqr_lqt* h, const double* mu) { return set_targets(h, mu, true); }

extern "C" int ilqr_lqt_solve_dp(ilqr_lqt* h) {
    if (!h) return 1;
    ilqr_ctx* c = h->ctx;
    if (!h->has_targets) return fail(c, "ilqr_lqt_solve_dp: set the targets first (ilqr_lqt_set_targets)");
    HIPCHK(c, hipSetDevice(c->device));
    launch_lqt_chain(h->dv, c->stream);
    HIPCHK(c, hipGetLastError());
    if (h->dv.chains == 1) {
        launch_lqt_affine(h->dv, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    h->dp_done = true;
    return 0;
}

extern "C" int ilqr_lqt_solve_lin_al(ilqr_lqt* h) {
    if (!h) return 1;
    ilqr_ctx* c = h->ctx;
    if (!h->dp_done && ilqr_lqt_solve_dp(h)) return 1;
    launch_lqt_rollout(h->dv, c->stream);
    HIPCHK(c, hipGetLastError());
    h->linal_done = true;
    return 0;
}

static int command(ilqr_lqt* h, int t, const double* x, double* u, bool dev) {
    if (!h) return 1;
    ilqr_ctx* c = h->ctx;
    if (!h->dp_done) return fail(c, kDpFirst);
    if (t < -1 || t > h->dv.N - 2)
        return fail(c, "ilqr_lqt_command: t must be in -1.." + std::to_string(h->dv.N - 2) + " (got " + std::to_string(t) + ")");
    if (!x || !u) return fail(c, "ilqr_lqt_command: null x or u");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nx = (size_t)h->dv.B * h->dv.n, nu = (size_t)h->dv.B * h->dv.m;
    const double* xs = x;
    double* us = u;
    if (!dev) {
        HIPCHK(c, hipMemcpyAsync(h->staging, x, nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
        xs = h->staging;
        us = h->staging + nx;
    }
    launch_lqt_command(h->dv, t + 1, xs, us, c->stream);
    HIPCHK(c, hipGetLastError());
    if (!dev) {
        HIPCHK(c, hipMemcpyAsync(u, us, nu * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}
extern "C" int ilqr_lqt_command(ilqr_lqt* h, int t, const double* x, double* u) { return command(h, t, x, u, false); }
extern "C" int ilqr_lqt_command_dev(ilqr_lqt* h, int t, const double* x, double* u) { return command(h, t, x, u, true); }

static int download(ilqr_lqt* h, bool ready, const char* first, const double* src, size_t n, double* dst, bool dev) {
    ilqr_ctx* c = h->ctx;
    if (!ready) return fail(c, first);
    if (!dst) return fail(c, "null output pointer");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dst, src, n * sizeof(double), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    if (!dev) HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
static size_t n_U(const ilqr_lqt* h) { return (size_t)h->dv.B * (h->dv.N - 1) * h->dv.m; }
static size_t n_X(const ilqr_lqt* h) { return (size_t)h->dv.B * h->dv.N * h->dv.n; }
extern "C" int ilqr_lqt_get_U(ilqr_lqt* h, double* U) { return h ? download(h, h->linal_done, kLinalFirst, h->dv.U, n_U(h), U, false) : 1; }
extern "C" int ilqr_lqt_get_U_dev(ilqr_lqt* h, double* U) { return h ? download(h, h->linal_done, kLinalFirst, h->dv.U, n_U(h), U, true) : 1; }
extern "C" int ilqr_lqt_get_X(ilqr_lqt* h, double* X) { return h ? download(h, h->linal_done, kLinalFirst, h->dv.X, n_X(h), X, false) : 1; }
extern "C" int ilqr_lqt_get_X_dev(ilqr_lqt* h, double* X) { return h ? download(h, h->linal_done, kLinalFirst, h->dv.X, n_X(h), X, true) : 1; }
extern "C" int ilqr_lqt_get_P(ilqr_lqt* h, double* P) {
    return h ? download(h, h->dp_done, kDpFirst, h->dv.P, (size_t)h->dv.chains * h->dv.N * h->dv.n * h->dv.n, P, false) : 1;
}
extern "C" int ilqr_lqt_get_d(ilqr_lqt* h, double* d) { return h ? download(h, h->dp_done, kDpFirst, h->dv.d, n_X(h), d, false) : 1; }
