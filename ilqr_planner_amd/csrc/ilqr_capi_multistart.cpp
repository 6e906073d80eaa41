// ilqr_capi_multistart.cpp -- C ABI (include/ilqr_hip.h): the calls that join instances (adopt, spread, select, get_at).
#include "ilqr_capi_internal.hpp"

using namespace ilqr_capi;

// ------------------------------------------------------------------------------------------------ multi-start
// The calls that join instances (include/ilqr_hip.h "multi-start"): every refusal first, then the launches of ilqr_multistart.hpp on the context's
// stream, charged to ILQR_PROF_OTHER.  Host forms stage their arrays, ints and doubles, in the problem's `staging` (Staging), and synchronise.

static int ms_groups(ilqr_ctx* c, const char* fn, int B, int S) {
    if (S < 1) return fail(c, std::string(fn) + ": group_size must be >= 1 (got " + std::to_string(S) + ")");
    if (B % S != 0) return fail(c, std::string(fn) + ": the batch (" + std::to_string(B) + ") is not a multiple of group_size (" + std::to_string(S) + ")");
    return 0;
}
// the index of a host-form call, checked against 0 .. B_src-1 before it is uploaded (the _dev forms cannot look: their kernels clamp)
static int ms_index(ilqr_ctx* c, const char* fn, const int* index, int n, int B_src) {
    for (int i = 0; i < n; i++)
        if (index[i] < 0 || index[i] >= B_src)
            return fail(c, std::string(fn) + ": index[" + std::to_string(i) + "] = " + std::to_string(index[i]) + " is outside 0 .. " + std::to_string(B_src - 1));
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
    const int* idx = index;
    Staging stg{c};
    if (!dev && (ms_index(c, fn, index, dst->B, src->B) || stg.lay(dst->staging, [&](Staging& s) { idx = s.take_in(index, (size_t)dst->B); }))) return 1;
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
    return dev ? 0 : stg.fetch();  // waits: the index array is the caller's
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
    Staging stg{c};
    if (!dev && stg.lay(p->staging, [&](Staging& s) {   // the kernel writes all three outputs
            if (score) dscore = s.take_in(score, (size_t)B);
            if (eligible) delig = s.take_in(eligible, (size_t)B);
            dwin = s.take_out(winner, (size_t)G);
            dbest = s.take_out(best, (size_t)G);
            dn = s.take_out(n_cand, (size_t)G);
        })) return 1;
    {
        ProfScope ps(c, ILQR_PROF_OTHER);
        launch_select_group(dscore, delig, p->bufs.status, G, S, dwin, dbest, dn, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    prof_mark(c, -1);
    return dev ? 0 : stg.fetch();
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
    if (!dev && ms_index(c, fn, index, n, p->B)) return 1;
    const int* idx = index;
    const int rx = p->T * p->udims.n_x, ru = (p->T - 1) * p->udims.n_u;
    double *dX = X, *dU = U, *dcost = cost;
    int *dit = iters, *dst = status;
    Staging stg{c};
    if (!dev && stg.lay(p->staging, [&](Staging& s) {
            idx = s.take_in(index, (size_t)n);
            if (X) dX = s.take_out(X, (size_t)n * rx);
            if (U) dU = s.take_out(U, (size_t)n * ru);
            if (cost) dcost = s.take_out(cost, (size_t)n);
            if (iters) dit = s.take_out(iters, (size_t)n);
            if (status) dst = s.take_out(status, (size_t)n);
        })) return 1;
    const Bufs& b = p->bufs;
    // one mark per launch that happens
    if (X) { ProfScope ps(c, ILQR_PROF_OTHER); launch_get_at(b.X[0], b.X[1], b.cur, idx, dX, n, p->B, p->Bp, rx, p->mapped ? &p->map.x : nullptr, c->stream); }
    if (U) { ProfScope ps(c, ILQR_PROF_OTHER); launch_get_at(b.U[0], b.U[1], b.cur, idx, dU, n, p->B, p->Bp, ru, p->mapped ? &p->map.u : nullptr, c->stream); }
    if (cost) { ProfScope ps(c, ILQR_PROF_OTHER); launch_get_at(b.cost, nullptr, nullptr, idx, dcost, n, p->B, p->Bp, 1, nullptr, c->stream); }
    if (iters) { ProfScope ps(c, ILQR_PROF_OTHER); launch_get_at_int(b.iters, idx, dit, n, p->B, c->stream); }
    if (status) { ProfScope ps(c, ILQR_PROF_OTHER); launch_get_at_int(b.status, idx, dst, n, p->B, c->stream); }
    HIPCHK(c, hipGetLastError());
    prof_mark(c, -1);
    return dev ? 0 : stg.fetch();
}
extern "C" int ilqr_problem_get_at(ilqr_problem* p, int n, const int* index, double* X, double* U, double* cost, int* iters, int* status) {
    return get_at(p, n, index, X, U, cost, iters, status, false);
}
extern "C" int ilqr_problem_get_at_dev(ilqr_problem* p, int n, const int* index, double* X, double* U, double* cost, int* iters, int* status) {
    return get_at(p, n, index, X, U, cost, iters, status, true);
}
