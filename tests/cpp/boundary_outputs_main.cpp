// The host / _dev pairs of the C ABI outside the closed loop give the same bytes whichever outputs are asked for and whichever memory the arrays
// are in: get_X / get_U / get_cost, track, get_at, select, adopt, the two clearance calls and obstacle_terms.  Every array of every call equals,
// byte for byte, the same array of the all-outputs host call.  Built with the host sources of the library (tests/tools/hostsim) under
// -fsanitize=address,undefined by tests/test_boundary_outputs_cpu.py: on that build a "device" buffer is host memory, so an overrun of a staging
// layout is seen by the sanitizer, and an overrun inside one of this program's own arrays by the guard bytes behind it; arrays a call does not
// ask for are not handed to the library and must stay poisoned.  The whole list of calls runs forward and then backward, so that every grow-only
// buffer is reused after a larger and after a smaller need.  argv[1] = Panda URDF, argv[2] = the four-joint URDF.  Prints the number of calls
// made (references apart); exit code 0 = all passed.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <memory>
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

enum { B = 4, T = 6, NKP = 2, GUARD = 64, MAX_OUT = 6 };
static const unsigned char GUARD_BYTE = 0xA5, POISON_BYTE = 0xC7;  // as a double -2.4e38.., as an int -9.4e8: no result is either

typedef std::vector<unsigned char> Bytes;

// One array handed to the library: n bytes and GUARD guard bytes behind them, in host memory or in memory of hipMalloc.
struct Arr {
    Bytes host;
    void* dev = nullptr;
    size_t n = 0;
    Arr() {}
    Arr(const Arr&) = delete;
    ~Arr() { if (dev) (void)hipFree(dev); }
    bool make(size_t n_, bool on_dev, const void* init = nullptr) {
        n = n_;
        host.assign(n + GUARD, GUARD_BYTE);
        if (init) std::memcpy(host.data(), init, n);
        else std::memset(host.data(), POISON_BYTE, n);
        if (!on_dev) return true;
        return hipMalloc(&dev, host.size()) == hipSuccess && hipMemcpy(dev, host.data(), host.size(), hipMemcpyHostToDevice) == hipSuccess;
    }
    void* ptr() { return dev ? dev : (void*)host.data(); }
    bool fetch() { return !dev || hipMemcpy(host.data(), dev, host.size(), hipMemcpyDeviceToHost) == hipSuccess; }
    bool guard_ok() const {
        for (size_t i = n; i < host.size(); i++)
            if (host[i] != GUARD_BYTE) return false;
        return true;
    }
    bool poisoned() const {  // every byte still as made
        for (size_t i = 0; i < n; i++)
            if (host[i] != POISON_BYTE) return false;
        return true;
    }
    bool has_poison(size_t esz) const {  // an element was not written
        for (size_t i = 0; i + esz <= n; i += esz) {
            bool all = true;
            for (size_t j = 0; j < esz; j++) all = all && host[i + j] == POISON_BYTE;
            if (all) return true;
        }
        return false;
    }
};

// The input arrays of one call, in the memory the call takes; checked unchanged afterwards.
struct Inputs {
    bool dev = false;
    std::vector<std::unique_ptr<Arr>> arrs;
    std::vector<Bytes> orig;
    bool failed = false;
    const void* add(const void* data, size_t bytes) {
        arrs.emplace_back(new Arr());
        orig.emplace_back((const unsigned char*)data, (const unsigned char*)data + bytes);
        if (!arrs.back()->make(bytes, dev, data)) failed = true;
        return arrs.back()->ptr();
    }
    template <class V>
    const V* add(const std::vector<V>& v) { return (const V*)add(v.data(), v.size() * sizeof(V)); }
    bool untouched() {
        for (size_t i = 0; i < arrs.size(); i++)
            if (!arrs[i]->fetch() || !arrs[i]->guard_ok() || std::memcmp(arrs[i]->host.data(), orig[i].data(), orig[i].size())) return false;
        return true;
    }
};

struct Spec { const char* name; size_t esz, n; };
struct Result { Bytes v[MAX_OUT]; };
// One call site with its inputs fixed: o[s] is the array of output s, null where the call does not ask for it
typedef std::function<int(void* const* o, bool dev, Inputs& in)> Fn;
struct Group {
    std::string what;
    std::vector<Spec> outs;
    Fn fn;
    Result ref;  // the all-outputs host call
};
struct Item { int group; unsigned want; bool dev; };

static ilqr_ctx* ctx;
static std::vector<Group> groups;
static std::vector<Item> items;
static int n_calls = 0;

static int run(Group& g, unsigned want, bool dev, Result& r) {
    const int ns = (int)g.outs.size();
    Arr out[MAX_OUT];
    void* o[MAX_OUT];
    for (int s = 0; s < ns; s++) {
        const bool w = (want >> s) & 1u;
        CHECK(out[s].make(g.outs[s].esz * g.outs[s].n, dev && w));
        o[s] = w ? out[s].ptr() : nullptr;
    }
    Inputs in;
    in.dev = dev;
    if (g.fn(o, dev, in)) { std::printf("FAILED: %s want %#x dev %d: %s\n", g.what.c_str(), want, (int)dev, ilqr_last_error(ctx)); return 1; }
    CHECK(!in.failed);
    if (dev) OK(ilqr_ctx_synchronize(ctx));
    for (int s = 0; s < ns; s++) {
        r.v[s].clear();
        CHECK(out[s].fetch());
        if (!out[s].guard_ok()) { std::printf("FAILED: guard behind %s overwritten (%s want %#x dev %d)\n", g.outs[s].name, g.what.c_str(), want, (int)dev); return 1; }
        if (!o[s]) {
            if (!out[s].poisoned()) { std::printf("FAILED: %s written though not asked for (%s want %#x dev %d)\n", g.outs[s].name, g.what.c_str(), want, (int)dev); return 1; }
            continue;
        }
        if (out[s].has_poison(g.outs[s].esz)) { std::printf("FAILED: %s not fully written (%s want %#x dev %d)\n", g.outs[s].name, g.what.c_str(), want, (int)dev); return 1; }
        r.v[s].assign(out[s].host.begin(), out[s].host.begin() + out[s].n);
    }
    if (!in.untouched()) { std::printf("FAILED: an input was written or overrun (%s want %#x dev %d)\n", g.what.c_str(), want, (int)dev); return 1; }
    return 0;
}

static int same(const Group& g, unsigned want, bool dev, const Result& got) {
    for (size_t s = 0; s < g.outs.size(); s++) {
        if (!((want >> s) & 1u)) continue;
        if (got.v[s].size() != g.ref.v[s].size() || std::memcmp(got.v[s].data(), g.ref.v[s].data(), got.v[s].size())) {
            std::printf("FAILED: %s differs from the all-outputs host call (%s want %#x dev %d)\n", g.outs[s].name, g.what.c_str(), want, (int)dev);
            return 1;
        }
    }
    return 0;
}

static void add_group(const std::string& what, std::vector<Spec> outs, const std::vector<unsigned>& wants, Fn fn) {
    groups.push_back({what, std::move(outs), std::move(fn), {}});
    for (unsigned w : wants)
        for (int dev = 0; dev < 2; dev++) items.push_back({(int)groups.size() - 1, w, dev != 0});
}
static std::vector<unsigned> subsets(int n) {
    std::vector<unsigned> v;
    for (unsigned m = 1; m < (1u << n); m++) v.push_back(m);
    return v;
}

// One chain's problems: `p` solved without obstacle terms, `dst` the destination of adopt, `pobs` solved with obstacle terms, without and with
// self pairs.
struct Prob {
    std::string name;
    ilqr_problem_desc d;
    int dof = 0;
    ilqr_problem *p = nullptr, *dst = nullptr, *pobs[2] = {nullptr, nullptr};
    std::vector<double> q0, U0, tg[NKP], q0d, U0d, tgd[NKP];  // the inputs of p (and pobs), and those dst is reset to before every adopt
    ilqr_clr_robot robot[2];
    std::vector<double> obs, X;  // the obstacle sets; p's plan (the trajectories of ilqr_clearance_trajectories)
};

static int give(ilqr_problem* q, const std::vector<double>& q0, const std::vector<double>* tg, const std::vector<double>& U0) {
    OK(ilqr_problem_set_init_state(q, q0.data(), nullptr));
    for (int k = 0; k < NKP; k++) OK(ilqr_problem_set_keypoint_targets(q, k, tg[k].data()));
    OK(ilqr_problem_set_controls(q, U0.data()));
    return 0;
}

static int put(void* dst, const std::vector<double>& v, bool dev) {
    CHECK(hipMemcpy(dst, v.data(), v.size() * sizeof(double), dev ? hipMemcpyHostToDevice : hipMemcpyHostToHost) == hipSuccess);
    return 0;
}

static int setup(Prob& P, const char* urdf_path, const char* base, const char* tip, int want_dof) {
    std::stringstream urdf;
    urdf << std::ifstream(urdf_path).rdbuf();
    ilqr_problem_desc& d = P.d;
    ilqr_desc_defaults(&d);
    if (ilqr_chain_from_urdf(urdf.str().c_str(), base, tip, nullptr, nullptr, &d, nullptr, nullptr)) {
        std::printf("FAILED: %s\n", ilqr_urdf_last_error());
        return 1;
    }
    CHECK(d.dof == want_dof);
    const int dof = P.dof = d.dof;
    d.kind = ILQR_SYS_POS_ORN; d.nb_deriv = 1; d.horizon = T; d.dt = 0.1;
    for (int i = 0; i < dof; i++) d.R_diag[i] = 1e-3;
    d.n_kp = NKP;
    d.kp_timestep[0] = 2; d.kp_timestep[1] = T - 1;
    ilqr_dims dm;
    CHECK(!ilqr_dims_of(&d, &dm) && dm.n_x == dof && dm.n_u == dof && dm.n_f == 7 && dm.n_Q == 6);
    for (int k = 0; k < NKP; k++)
        for (int i = 0; i < 6; i++) d.kp_Q[k][i * 6 + i] = i < 3 ? 100.0 : 10.0;

    // start configurations; the keypoint targets are poses of other configurations
    P.q0.resize((size_t)B * dof); P.q0d.resize((size_t)B * dof);
    for (int b = 0; b < B; b++)
        for (int i = 0; i < dof; i++) {
            P.q0[b * dof + i] = 0.2 * ((b + 2 * i) % 5 - 2);
            P.q0d[b * dof + i] = P.q0[b * dof + i] + 0.05 * (1 + (b + i) % 3);
        }
    for (int k = 0; k < NKP; k++)
        for (int v = 0; v < 2; v++) {
            std::vector<double> qt((size_t)B * dof), pos((size_t)B * 3), quat((size_t)B * 4);
            for (int b = 0; b < B; b++)
                for (int i = 0; i < dof; i++) qt[b * dof + i] = 0.3 * ((3 * b + i + 2 * k + 4 * v) % 7 - 3);
            OK(ilqr_fk_batch(ctx, &d, B, qt.data(), pos.data(), quat.data(), nullptr));
            std::vector<double>& tg = v ? P.tgd[k] : P.tg[k];
            tg.resize((size_t)B * 7);
            for (int b = 0; b < B; b++) {
                for (int i = 0; i < 3; i++) tg[b * 7 + i] = pos[b * 3 + i];
                for (int i = 0; i < 4; i++) tg[b * 7 + 3 + i] = quat[b * 4 + i];
            }
        }
    P.U0.assign((size_t)B * (T - 1) * dof, 0.0);
    P.U0d.resize(P.U0.size());
    for (size_t j = 0; j < P.U0d.size(); j++) P.U0d[j] = 0.01 * (double)((int)((3 * j + j / 5) % 9) - 4);

    // 3 spheres on links behind the first joint, a middle joint and at the tool; 1 plane; 2 obstacles per set; the self pairs (0, 2), (1, 2)
    std::vector<int> js(dof, -1);
    for (int s = 0; s < d.n_seg; s++)
        if (d.seg_joint[s] >= 0) js[d.seg_joint[s]] = s;
    for (int v = 0; v < 2; v++) {
        ilqr_clr_robot& rb = P.robot[v];
        std::memset(&rb, 0, sizeof(rb));
        rb.n_sph = 3;
        rb.sph_link[0] = js[0]; rb.sph_link[1] = js[dof / 2]; rb.sph_link[2] = d.n_seg - 1;
        for (int i = 0; i < 3; i++) { rb.sph_c[i][0] = 0.01 * i; rb.sph_c[i][1] = -0.02; rb.sph_c[i][2] = 0.03 * (i + 1); rb.sph_r[i] = 0.04 + 0.01 * i; }
        rb.n_planes = 1;
        rb.plane_n[0][2] = 1.0; rb.plane_d[0] = -0.25;
        if (v) { rb.n_self = 2; rb.self_pair[0][0] = 0; rb.self_pair[0][1] = 2; rb.self_pair[1][0] = 1; rb.self_pair[1][1] = 2; }
    }
    P.obs.resize((size_t)(B / 2) * 2 * 4);
    for (int s = 0; s < B / 2; s++)
        for (int j = 0; j < 2; j++) {
            double* o = &P.obs[((size_t)s * 2 + j) * 4];
            o[0] = 0.3 + 0.1 * s; o[1] = -0.2 + 0.3 * j; o[2] = 0.4 + 0.1 * (s + j); o[3] = 0.08 + 0.02 * j;
        }

    OK(ilqr_problem_create(ctx, &d, B, &P.p));
    OK(ilqr_problem_create(ctx, &d, B, &P.dst));
    if (give(P.p, P.q0, P.tg, P.U0)) return 1;
    OK(ilqr_solve_recursive(P.p, 2, 1, 0));
    P.X.resize((size_t)B * T * dof);
    OK(ilqr_problem_get_X(P.p, P.X.data()));
    for (int v = 0; v < 2; v++) {
        OK(ilqr_problem_create(ctx, &d, B, &P.pobs[v]));
        if (give(P.pobs[v], P.q0, P.tg, P.U0)) return 1;
        const ilqr_clr_world w = {P.obs.data(), B / 2, 2, 2, 0.6, 0};
        OK(ilqr_problem_set_obstacles(P.pobs[v], &P.robot[v], &w, 5.0));
        OK(ilqr_solve_recursive(P.pobs[v], 2, 1, 0));
    }
    return 0;
}

static void add_calls(Prob& P) {
    Prob* q = &P;
    const size_t nx = P.dof, nu = P.dof, dof = P.dof;
    const std::string nm = P.name + " ";
    const size_t D = sizeof(double), I = sizeof(int);
    add_group(nm + "get_X", {{"X", D, B * T * nx}}, {1}, [q](void* const* o, bool dev, Inputs&) {
        return dev ? ilqr_problem_get_X_dev(q->p, (double*)o[0]) : ilqr_problem_get_X(q->p, (double*)o[0]);
    });
    add_group(nm + "get_U", {{"U", D, B * (T - 1) * nu}}, {1}, [q](void* const* o, bool dev, Inputs&) {
        return dev ? ilqr_problem_get_U_dev(q->p, (double*)o[0]) : ilqr_problem_get_U(q->p, (double*)o[0]);
    });
    add_group(nm + "get_cost", {{"cost", D, B}}, {1}, [q](void* const* o, bool dev, Inputs&) {
        return dev ? ilqr_problem_get_cost_dev(q->p, (double*)o[0]) : ilqr_problem_get_cost(q->p, (double*)o[0]);
    });
    for (int k : {0, T - 2})
        for (int ff = 0; ff < 2; ff++)
            add_group(nm + "track k " + std::to_string(k) + " ff " + std::to_string(ff), {{"u_out", D, B * nu}}, {1}, [q, k, ff, nx](void* const* o, bool dev, Inputs& in) {
                std::vector<double> xm((size_t)B * nx);
                for (size_t j = 0; j < xm.size(); j++) xm[j] = q->X[(j / nx) * T * nx + (size_t)k * nx + j % nx] + 0.02 * (double)((int)(j % 5) - 2);
                const double* x = in.add(xm);
                return dev ? ilqr_problem_track_dev(q->p, k, x, ff, (double*)o[0]) : ilqr_problem_track(q->p, k, x, ff, (double*)o[0]);
            });
    {
        const int n = 3;
        add_group(nm + "get_at", {{"X", D, n * T * nx}, {"U", D, n * (T - 1) * nu}, {"cost", D, (size_t)n}, {"iters", I, (size_t)n}, {"status", I, (size_t)n}}, subsets(5),
                  [q](void* const* o, bool dev, Inputs& in) {
                      const int* idx = in.add(std::vector<int>{2, 0, 2});
                      return dev ? ilqr_problem_get_at_dev(q->p, 3, idx, (double*)o[0], (double*)o[1], (double*)o[2], (int*)o[3], (int*)o[4])
                                 : ilqr_problem_get_at(q->p, 3, idx, (double*)o[0], (double*)o[1], (double*)o[2], (int*)o[3], (int*)o[4]);
                  });
    }
    for (int S : {2, 4})
        for (int sc = 0; sc < 2; sc++)
            for (int el = 0; el < 2; el++) {
                const size_t G = B / S;
                add_group(nm + "select S " + std::to_string(S) + " score " + std::to_string(sc) + " eligible " + std::to_string(el),
                          {{"winner", I, G}, {"best", D, G}, {"n_candidates", I, G}}, subsets(3), [q, S, sc, el](void* const* o, bool dev, Inputs& in) {
                              const double* score = sc ? in.add(std::vector<double>{0.5, -1.25, 3.0, -1.25}) : nullptr;
                              const int* elig = el ? in.add(std::vector<int>{1, 0, 1, 1}) : nullptr;
                              return dev ? ilqr_problem_select_dev(q->p, S, score, elig, (int*)o[0], (double*)o[1], (int*)o[2])
                                         : ilqr_problem_select(q->p, S, score, elig, (int*)o[0], (double*)o[1], (int*)o[2]);
                          });
            }
    for (int what : {ILQR_ADOPT_STATE, ILQR_ADOPT_TARGETS, ILQR_ADOPT_CONTROLS0, ILQR_ADOPT_CONTROLS, ILQR_ADOPT_STATE | ILQR_ADOPT_TARGETS | ILQR_ADOPT_CONTROLS})
        add_group(nm + "adopt what " + std::to_string(what), {{"X", D, B * T * nx}, {"U", D, B * (T - 1) * nu}}, {3}, [q, what, nx, nu](void* const* o, bool dev, Inputs& in) -> int {
            if (give(q->dst, q->q0d, q->tgd, q->U0d)) return 1;
            const int* idx = in.add(std::vector<int>{3, 1, 1, 0});
            if (dev ? ilqr_problem_adopt_dev(q->dst, q->p, idx, what) : ilqr_problem_adopt(q->dst, q->p, idx, what)) return 1;
            std::vector<double> X((size_t)B * T * nx), U((size_t)B * (T - 1) * nu);
            if (ilqr_solve_recursive(q->dst, 0, 1, 0) || ilqr_problem_get_X(q->dst, X.data()) || ilqr_problem_get_U(q->dst, U.data())) return 1;
            return put(o[0], X, dev) || put(o[1], U, dev);
        });
    for (int traj = 0; traj < 2; traj++)
        for (int v = 0; v < 2; v++)
            add_group(nm + (traj ? "clearance_trajectories" : "problem_clearance") + " self " + std::to_string(v),
                      {{"clr", D, (size_t)B * T}, {"clr_min", D, B}, {"clr_at", I, 3 * B}, {"n_below", I, B}, {"eligible", I, B}, {"stats", D, (B / 2) * ILQR_CLR_STATS}}, subsets(6),
                      [q, traj, v](void* const* o, bool dev, Inputs& in) {
                          const ilqr_clr_world w = {in.add(q->obs), B / 2, 2, 2, 0.2, 2};
                          const ilqr_clr_out out = {(double*)o[0], (double*)o[1], (int*)o[2], (int*)o[3], (int*)o[4], (double*)o[5]};
                          if (!traj) return dev ? ilqr_problem_clearance_dev(q->p, &q->robot[v], &w, &out) : ilqr_problem_clearance(q->p, &q->robot[v], &w, &out);
                          const double* X = in.add(q->X);
                          return dev ? ilqr_clearance_trajectories_dev(ctx, &q->d, B, T, X, &q->robot[v], &w, &out)
                                     : ilqr_clearance_trajectories(ctx, &q->d, B, T, X, &q->robot[v], &w, &out);
                      });
    for (int v = 0; v < 2; v++)
        add_group(nm + "obstacle_terms self " + std::to_string(v), {{"cost", D, (size_t)B * T}, {"lx", D, B * T * dof}, {"lxx", D, B * T * dof * dof}}, subsets(3),
                  [q, v](void* const* o, bool dev, Inputs&) {
                      return dev ? ilqr_problem_obstacle_terms_dev(q->pobs[v], (double*)o[0], (double*)o[1], (double*)o[2])
                                 : ilqr_problem_obstacle_terms(q->pobs[v], (double*)o[0], (double*)o[1], (double*)o[2]);
                  });
}

static int run_item(const Item& it) {
    Group& g = groups[it.group];
    Result r;
    if (run(g, it.want, it.dev, r) || same(g, it.want, it.dev, r)) return 1;
    n_calls++;
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    CHECK(!ilqr_ctx_create(0, &ctx));
    OK(ilqr_ctx_set_crosscheck(ctx, 1, 0, 0, 0, 0, 0));  // the host build holds the generic kernels only
    static Prob probs[2];
    probs[0].name = "panda"; probs[1].name = "gen4";
    if (setup(probs[0], argv[1], "panda_link0", "panda_tip", 7) || setup(probs[1], argv[2], "g4_base", "g4_tip", 4)) return 1;
    for (Prob& P : probs) add_calls(P);
    // the references: the all-outputs host call of every call site
    for (Group& g : groups)
        if (run(g, (1u << g.outs.size()) - 1, false, g.ref)) return 1;
    for (size_t i = 0; i < items.size(); i++)
        if (run_item(items[i])) return 1;
    for (size_t i = items.size(); i-- > 0;)
        if (run_item(items[i])) return 1;
    for (Prob& P : probs) {
        for (ilqr_problem* p : {P.p, P.dst, P.pobs[0], P.pobs[1]}) ilqr_problem_destroy(p);
    }
    ilqr_ctx_destroy(ctx);
    std::printf("call sites: %d\n", (int)groups.size());
    std::printf("cases: %d\n", n_calls);
    std::printf("ok\n");
    return 0;
}
