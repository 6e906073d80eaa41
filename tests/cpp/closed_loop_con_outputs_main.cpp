// Every subset of the outputs that ilqr_problem_closed_loop_report_con and ilqr_problem_closed_loop_cov_con add gives the same bytes: what a
// call returns does not depend on which other outputs it was asked for -- with every output of the older struct beside them and with none --
// nor on whether the arrays are the caller's host memory or device pointers.  The pattern of closed_loop_outputs_main.cpp: built with the host
// sources of the library (tests/tools/hostsim) under -fsanitize=address,undefined by tests/test_closed_loop_con_outputs_cpu.py; on that build a
// "device" buffer is host memory, so an overrun of the staging layout or of a workspace (con_max | con_steps, kp_err | lim_cost) is seen by the
// sanitizer, and an overrun inside one of this program's own buffers by the guard words behind it.  argv[1] = URDF path.  Prints the number of
// calls made; exit code 0 = all passed.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ilqr_hip.h"

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { std::printf("FAILED: %s (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)
#define OK(call)                                                                                                      \
    do {                                                                                                              \
        if (call) { std::printf("FAILED: %s (line %d): %s\n", #call, __LINE__, ilqr_last_error(ctx)); return 1; }     \
    } while (0)

enum { B = 3, T = 6, S = 2, NKP = 2, M = 3, GUARD = 8 };
enum Slot { COST, STATS, KP_ERR, KP_STATS, LIM_COST, OUTCOME, CON_MAX, CON_STEPS, CON_STATS, OUTCOME_CON,   // report_con
            SIGMA, KP_SIGMA, KP_VAR, U_VAR, LIM_Z, CON_VAR, CON_Z,                                          // cov_con
            N_SLOT };
enum Entry { REPORT_CON, COV_CON };
static const char* const SLOT_NAME[N_SLOT] = {"cost", "stats", "kp_err", "kp_stats", "lim_cost", "outcome", "con_max", "con_steps", "con_stats", "outcome_con",
                                              "Sigma", "kp_Sigma", "kp_var", "u_var", "lim_z", "con_var", "con_z"};
static const double GUARD_WORD = -7.25e300, POISON = 4.5e299;
static const double CON_TOL = 0.05;

static size_t slot_elems[N_SLOT];

// One array handed to the library: n doubles and GUARD guard words behind them, in host memory or in memory of hipMalloc.
struct Arr {
    std::vector<double> host;
    double* dev = nullptr;
    size_t n = 0;
    ~Arr() { if (dev) (void)hipFree(dev); }
    bool make(size_t n_, bool on_dev, const double* init = nullptr) {
        n = n_;
        host.assign(n + GUARD, GUARD_WORD);
        for (size_t i = 0; i < n; i++) host[i] = init ? init[i] : POISON;
        if (!on_dev) return true;
        return hipMalloc((void**)&dev, host.size() * sizeof(double)) == hipSuccess &&
               hipMemcpy(dev, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    }
    double* ptr() { return dev ? dev : host.data(); }
    bool fetch() { return !dev || hipMemcpy(host.data(), dev, host.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess; }
    bool guard_ok() const {
        for (size_t i = n; i < host.size(); i++)
            if (std::memcmp(&host[i], &GUARD_WORD, sizeof(double))) return false;
        return true;
    }
};

struct Call {
    Entry entry;
    unsigned want;  // bit per Slot
    bool x0, w, noise, dev;
};
struct Result { std::vector<double> v[N_SLOT]; };

static ilqr_ctx* ctx;
static ilqr_problem* prob;
static std::vector<double> x0_in, w_in;
static ilqr_noise noise_in;
static ilqr_cl_tol tol_in;
static double sigma_w[7], sigma_x0[7];
static int n_calls = 0;

static bool any(const unsigned want, int lo, int hi) {
    for (int s = lo; s <= hi; s++)
        if ((want >> s) & 1u) return true;
    return false;
}

static int run(const Call& c, Result& r) {
    Arr out[N_SLOT], x0, w;
    double* o[N_SLOT];
    for (int s = 0; s < N_SLOT; s++) {
        o[s] = nullptr;
        if (!((c.want >> s) & 1u)) continue;
        CHECK(out[s].make(slot_elems[s], c.dev));
        o[s] = out[s].ptr();
    }
    if (c.x0) CHECK(x0.make(x0_in.size(), c.dev, x0_in.data()));
    if (c.w) CHECK(w.make(w_in.size(), c.dev, w_in.data()));
    const double *px0 = c.x0 ? x0.ptr() : nullptr, *pw = c.w ? w.ptr() : nullptr;
    const ilqr_noise* nz = c.noise ? &noise_in : nullptr;
    int rc = 1;
    if (c.entry == REPORT_CON) {
        const ilqr_cl_report rep = {o[KP_ERR], o[KP_STATS], o[LIM_COST], o[OUTCOME]};
        const ilqr_cl_con con = {o[CON_MAX], o[CON_STEPS], o[CON_STATS], o[OUTCOME_CON]};
        // a null struct where it asks for nothing: both forms of "not asked for" are exercised
        const ilqr_cl_report* prep = any(c.want, KP_ERR, OUTCOME) ? &rep : nullptr;
        const ilqr_cl_con* pcon = any(c.want, CON_MAX, OUTCOME_CON) ? &con : nullptr;
        rc = c.dev ? ilqr_problem_closed_loop_report_con_dev(prob, S, nz, px0, pw, 1, &tol_in, o[COST], o[STATS], prep, CON_TOL, pcon)
                   : ilqr_problem_closed_loop_report_con(prob, S, nz, px0, pw, 1, &tol_in, o[COST], o[STATS], prep, CON_TOL, pcon);
    } else {
        const ilqr_cl_cov cov = {o[SIGMA], o[KP_SIGMA], o[KP_VAR], o[U_VAR], o[LIM_Z]};
        const ilqr_cl_cov_con con = {o[CON_VAR], o[CON_Z]};
        const ilqr_cl_cov* pcov = any(c.want, SIGMA, LIM_Z) ? &cov : nullptr;
        const ilqr_cl_cov_con* pcon = any(c.want, CON_VAR, CON_Z) ? &con : nullptr;
        rc = c.dev ? ilqr_problem_closed_loop_cov_con_dev(prob, sigma_w, sigma_x0, pcov, pcon) : ilqr_problem_closed_loop_cov_con(prob, sigma_w, sigma_x0, pcov, pcon);
    }
    if (rc) { std::printf("FAILED: entry %d want %#x dev %d: %s\n", (int)c.entry, c.want, (int)c.dev, ilqr_last_error(ctx)); return 1; }
    if (c.dev) OK(ilqr_ctx_synchronize(ctx));
    n_calls++;
    for (int s = 0; s < N_SLOT; s++) {
        r.v[s].clear();
        if (!o[s]) continue;
        CHECK(out[s].fetch());
        if (!out[s].guard_ok()) { std::printf("FAILED: guard behind %s overwritten (entry %d want %#x dev %d)\n", SLOT_NAME[s], (int)c.entry, c.want, (int)c.dev); return 1; }
        r.v[s].assign(out[s].host.begin(), out[s].host.begin() + out[s].n);
        for (double d : r.v[s])
            if (!std::memcmp(&d, &POISON, sizeof(double))) { std::printf("FAILED: %s not fully written (entry %d want %#x dev %d)\n", SLOT_NAME[s], (int)c.entry, c.want, (int)c.dev); return 1; }
    }
    // the inputs are read only, and nothing is written behind them
    CHECK(x0.fetch() && w.fetch() && x0.guard_ok() && w.guard_ok());
    if (c.x0) CHECK(!std::memcmp(x0.host.data(), x0_in.data(), x0_in.size() * sizeof(double)));
    if (c.w) CHECK(!std::memcmp(w.host.data(), w_in.data(), w_in.size() * sizeof(double)));
    return 0;
}

// every array of `got` equals the same array of `ref` byte for byte
static int same(const Call& c, const Result& got, const Result& ref, const char* what) {
    for (int s = 0; s < N_SLOT; s++) {
        if (got.v[s].empty()) continue;
        if (got.v[s].size() != ref.v[s].size() || std::memcmp(got.v[s].data(), ref.v[s].data(), got.v[s].size() * sizeof(double))) {
            std::printf("FAILED: %s differs from %s (entry %d want %#x x0 %d w %d noise %d dev %d)\n", SLOT_NAME[s], what, (int)c.entry, c.want, (int)c.x0,
                        (int)c.w, (int)c.noise, (int)c.dev);
            return 1;
        }
    }
    return 0;
}

// the subsets `wants` of one entry point with one set of inputs: host and device call of each against the all-outputs host call
static int sweep(Entry entry, unsigned all, const std::vector<unsigned>& wants, bool x0, bool w, bool noise) {
    Result ref, host, dev;
    const Call full = {entry, all, x0, w, noise, false};
    bool have_ref = false;
    for (unsigned want : wants) {
        if (want != all) continue;
        if (run(full, ref)) return 1;
        have_ref = true;
    }
    CHECK(have_ref);
    for (unsigned want : wants) {
        Call c = {entry, want, x0, w, noise, false};
        if (want == all) host = ref;
        else if (run(c, host) || same(c, host, ref, "the all-outputs call")) return 1;
        c.dev = true;
        if (run(c, dev) || same(c, dev, ref, "the all-outputs call") || same(c, dev, host, "its host twin")) return 1;
        for (int s = 0; s < N_SLOT; s++) CHECK(dev.v[s].size() == host.v[s].size());
    }
    return 0;
}

static unsigned bit(int s) { return 1u << s; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::stringstream urdf;
    urdf << std::ifstream(argv[1]).rdbuf();
    ilqr_problem_desc d;
    ilqr_desc_defaults(&d);
    double lo[ILQR_MAX_SEG], up[ILQR_MAX_SEG];
    if (ilqr_chain_from_urdf(urdf.str().c_str(), "panda_link0", "panda_tip", nullptr, nullptr, &d, lo, up)) {
        std::printf("FAILED: %s\n", ilqr_urdf_last_error());
        return 1;
    }
    CHECK(d.dof == 7);
    d.kind = ILQR_SYS_POS_ORN; d.nb_deriv = 1; d.horizon = T; d.dt = 0.1;
    for (int i = 0; i < 7; i++) d.R_diag[i] = 1e-3;
    d.limits_set = 1; d.penalty = 1.0;
    for (int i = 0; i < 7; i++) { d.state_max[i] = up[i]; d.state_min[i] = lo[i]; d.limit_weight[i] = 1; }
    d.n_kp = NKP;
    d.kp_timestep[0] = 2; d.kp_timestep[1] = T - 1;
    ilqr_dims dm;
    CHECK(!ilqr_dims_of(&d, &dm) && dm.n_x == 7 && dm.n_u == 7 && dm.n_f == 7 && dm.n_Q == 6);
    for (int k = 0; k < NKP; k++)
        for (int i = 0; i < 6; i++) d.kp_Q[k][i * 6 + i] = i < 3 ? 100.0 : 10.0;
    CHECK(!ilqr_ctx_create(0, &ctx));
    OK(ilqr_ctx_set_crosscheck(ctx, 1, 0, 0, 0, 0, 0));  // the host build holds the generic kernels only
    OK(ilqr_problem_create(ctx, &d, B, &prob));

    // start configurations inside the limits; the keypoint targets are poses of other configurations
    double q0[B][7], qt[NKP][B][7], tg[B][7], pos[B][3], quat[B][4];
    for (int b = 0; b < B; b++)
        for (int i = 0; i < 7; i++) {
            const double mid = 0.5 * (lo[i] + up[i]), half = 0.5 * (up[i] - lo[i]);
            q0[b][i] = mid + half * 0.3 * ((b + 2 * i) % 5 - 2) / 2.0;
            for (int k = 0; k < NKP; k++) qt[k][b][i] = mid + half * 0.4 * ((3 * b + i + 2 * k) % 7 - 3) / 3.0;
        }
    OK(ilqr_problem_set_init_state(prob, &q0[0][0], nullptr));
    for (int k = 0; k < NKP; k++) {
        OK(ilqr_fk_batch(ctx, &d, B, &qt[k][0][0], &pos[0][0], &quat[0][0], nullptr));
        for (int b = 0; b < B; b++) {
            for (int i = 0; i < 3; i++) tg[b][i] = pos[b][i];
            for (int i = 0; i < 4; i++) tg[b][3 + i] = quat[b][i];
        }
        OK(ilqr_problem_set_keypoint_targets(prob, k, &tg[0][0]));
    }
    const std::vector<double> U0((size_t)B * (T - 1) * 7, 0.0);
    OK(ilqr_problem_set_controls(prob, U0.data()));
    // three rows on [x; u]: a joint bound, a mixed state / control row and a control bound, placed so that some executions cross them
    double Arows[M][14] = {}, brows[M] = {0.0, 0.1, 0.3};
    Arows[0][1] = 1.0;
    brows[0] = q0[1][1];
    for (int i = 0; i < 7; i++) { Arows[1][i] = 0.1 * (i - 3); Arows[1][7 + i] = 0.05 * (3 - i); }
    Arows[2][7 + 2] = -1.0;
    OK(ilqr_problem_set_constraints(prob, M, 0, &Arows[0][0], brows, nullptr));
    OK(ilqr_solve_al(prob, 2, 1, 0.5, 1.5, 1, 0));

    const size_t n = (size_t)B * S;
    slot_elems[COST] = n; slot_elems[STATS] = (size_t)B * ILQR_CL_STATS; slot_elems[KP_ERR] = n * NKP * ILQR_KP_ERR;
    slot_elems[KP_STATS] = (size_t)B * NKP * ILQR_KP_STATS; slot_elems[LIM_COST] = n; slot_elems[OUTCOME] = (size_t)B * ILQR_CL_OUTCOME;
    slot_elems[CON_MAX] = n; slot_elems[CON_STEPS] = n; slot_elems[CON_STATS] = (size_t)B * ILQR_CL_CON_STATS;
    slot_elems[OUTCOME_CON] = (size_t)B * ILQR_CL_OUTCOME_CON;
    slot_elems[SIGMA] = (size_t)B * T * 49; slot_elems[KP_SIGMA] = (size_t)B * NKP * 49; slot_elems[KP_VAR] = (size_t)B * NKP * ILQR_CL_COV_KP;
    slot_elems[U_VAR] = (size_t)B * (T - 1) * 7; slot_elems[LIM_Z] = B; slot_elems[CON_VAR] = (size_t)B * (T - 1) * M; slot_elems[CON_Z] = B;

    // the caller's start states (the plan's start, moved; some beyond a limit) and disturbances
    x0_in.resize(n * 7);
    for (size_t g = 0; g < n; g++)
        for (int i = 0; i < 7; i++) x0_in[g * 7 + i] = q0[g / S][i] + 0.05 * (double)((int)((g + 3 * i) % 7) - 3) + (g == 1 && i == 0 ? 4.0 : 0.0);
    w_in.resize(n * (T - 1) * 7);
    for (size_t j = 0; j < w_in.size(); j++) w_in[j] = 0.01 * (double)((int)((5 * j + j / 7) % 11) - 5);
    std::memset(&noise_in, 0, sizeof(noise_in));
    noise_in.seed = 0x1234abcd5678ull; noise_in.instance_offset = 5; noise_in.sample_offset = 9;
    for (int i = 0; i < 7; i++) { noise_in.sigma_w[i] = 0.02 * (i % 3); noise_in.sigma_x0[i] = 0.1; sigma_w[i] = 0.01 * (i % 3); sigma_x0[i] = 0.05; }
    for (int k = 0; k < ILQR_MAX_KP; k++)
        for (int g = 0; g < ILQR_KP_ERR; g++) tol_in.kp_tol[k][g] = g == ILQR_KP_ERR_POS ? 0.3 : g == ILQR_KP_ERR_ORN ? 1.0 : -1.0;
    tol_in.lim_tol = 0.0;

    // ilqr_problem_closed_loop_report_con: every subset of {con_max, con_steps, con_stats, outcome_con}, beside every older output and beside
    // none of them (the empty call is refused); once with the draw (around the caller's x0), once with the caller's w
    {
        const unsigned old_all = bit(COST) | bit(STATS) | bit(KP_ERR) | bit(KP_STATS) | bit(LIM_COST) | bit(OUTCOME);
        std::vector<unsigned> wants;
        for (unsigned old = 0; old < 2; old++)
            for (unsigned m = 0; m < 16; m++) {
                const unsigned want = (old ? old_all : 0) | (m << CON_MAX);
                if (want) wants.push_back(want);
            }
        const unsigned all = old_all | (15u << CON_MAX);
        if (sweep(REPORT_CON, all, wants, true, false, true)) return 1;
        if (sweep(REPORT_CON, all, wants, false, true, false)) return 1;
    }
    const int after_report = n_calls;
    // ilqr_problem_closed_loop_cov_con: every subset of {con_var, con_z}, beside every output of ilqr_cl_cov and beside none
    {
        const unsigned old_all = bit(SIGMA) | bit(KP_SIGMA) | bit(KP_VAR) | bit(U_VAR) | bit(LIM_Z);
        std::vector<unsigned> wants;
        for (unsigned old = 0; old < 2; old++)
            for (unsigned m = 0; m < 4; m++) {
                const unsigned want = (old ? old_all : 0) | (m << CON_VAR);
                if (want) wants.push_back(want);
            }
        if (sweep(COV_CON, old_all | (3u << CON_VAR), wants, false, false, false)) return 1;
    }
    ilqr_problem_destroy(prob);
    ilqr_ctx_destroy(ctx);
    std::printf("calls: report_con %d cov_con %d\n", after_report, n_calls - after_report);
    std::printf("cases: %d\n", n_calls);
    std::printf("ok\n");
    return 0;
}
