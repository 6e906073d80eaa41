// ilqr_capi_clearance.cpp -- C ABI (include/ilqr_hip.h): clearance of plans and trajectories, and the obstacle terms of the stage cost.
#include "ilqr_capi_internal.hpp"

using namespace ilqr_capi;

// ------------------------------------------------------------------------------------------------ clearance
// include/ilqr_hip.h "clearance": every refusal first, then the three launches of ilqr_clearance.hpp on the context's stream, charged to
// ILQR_PROF_OTHER.  The geometry buffer, the workspace (12 bytes per (trajectory, step)) and the staging of the host forms (DevScratch, Staging) belong to the context
// and only grow; the geometry is uploaded when it differs from the one the buffer holds.

struct ClrState {
    ClrGeom host;        // what `geom` holds
    bool have = false;
    DevScratch geom, ws, io;  // the geometry block, the workspace, the staging of the host forms
    DevScratch cov[2];        // ilqr_problem_closed_loop_cov_clr: Sigma where the caller does not ask for it, the keys of k_cov_clr
};

void ilqr_capi::clr_release(ilqr_ctx* c) {
    if (!c->clr) return;
    c->clr->geom.release(); c->clr->ws.release(); c->clr->io.release(); c->clr->cov[0].release(); c->clr->cov[1].release();
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

int ilqr_capi::clr_check_world(ilqr_ctx* c, const std::string& fn, const ilqr_problem_desc& d, int n, int T, const ilqr_clr_robot* rb,
                               const ilqr_clr_world* w, bool dev) {
    return clr_check(c, fn, d, n, T, rb, w, nullptr, dev, false);
}

int ilqr_capi::clr_bind_geom(ilqr_ctx* c, const ilqr_problem_desc& d, const ilqr_clr_robot& rb, const ClrGeom** geom, int* n_anchor) {
    if (!c->clr) c->clr = new ClrState();
    ClrState& cs = *c->clr;
    ClrGeom g;
    clr_fill_geom(d, rb, g);
    if (!cs.have || std::memcmp(&g, &cs.host, sizeof(g)) != 0) {   // kernels in flight may read the old one; the copy's source must outlive it
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (cs.geom.reserve(c, sizeof(ClrGeom))) return 1;
        cs.host = g;
        cs.have = false;
        HIPCHK(c, hipMemcpyAsync(cs.geom.ptr, &cs.host, sizeof(ClrGeom), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        cs.have = true;
    }
    *geom = (const ClrGeom*)cs.geom.ptr;
    *n_anchor = g.n_anchor;
    return 0;
}

DevScratch& ilqr_capi::clr_cov_scratch(ilqr_ctx* c, int which) {
    if (!c->clr) c->clr = new ClrState();
    return c->clr->cov[which];
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
    ClrArgs a;
    std::memset(&a, 0, sizeof(a));
    if (clr_bind_geom(c, d, *rb, &a.geom, &a.n_anchor)) return 1;
    ClrState& cs = *c->clr;
    const size_t nT = (size_t)n * (size_t)T;
    if (cs.ws.reserve(c, nT * 12)) return 1;
    a.n = n; a.T = T; a.n_obs = w->n_obs; a.traj_per_set = w->traj_per_set;
    a.ws_clr = (double*)cs.ws.ptr;
    a.ws_code = (int*)(a.ws_clr + nT);
    for (int j = 0; j < DOF; j++) a.qrow[j] = j < d.dof ? (p ? p->map.x.dev[j] : j) : 0;
    a.obs = w->obs;
    const double* dX = X;
    ilqr_clr_out o = *out_;
    const int n_groups = out_->stats ? n / w->stats_group : 0;
    const size_t n_obs_all = (size_t)w->n_sets * (size_t)w->n_obs * 4, nX = p ? 0 : nT * (size_t)ud.n_x;
    Staging stg{c};
    if (!dev && stg.lay(cs.io, [&](Staging& s) {
            if (!p) dX = s.take_in(X, nX);
            if (n_obs_all) a.obs = s.take_in(w->obs, n_obs_all);
            if (out_->clr) o.clr = s.take_out(out_->clr, nT);
            if (out_->clr_min) o.clr_min = s.take_out(out_->clr_min, (size_t)n);
            if (out_->stats) o.stats = s.take_out(out_->stats, (size_t)n_groups * ILQR_CLR_STATS);
            if (out_->clr_at) o.clr_at = s.take_out(out_->clr_at, (size_t)3 * n);
            if (out_->n_below) o.n_below = s.take_out(out_->n_below, (size_t)n);
            if (out_->eligible) o.eligible = s.take_out(out_->eligible, (size_t)n);
        })) return 1;
    {
        ProfScope ps(c, ILQR_PROF_OTHER);
        if (p) launch_clr_plan(p->bufs.X[0], p->bufs.X[1], p->bufs.cur, p->dims.n_x, p->Bp, a, c->stream);
        else launch_clr_traj(dX, ud.n_x, a, c->stream);
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
    return dev ? 0 : stg.fetch();
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
    Staging stg{c};
    if (!dev && stg.lay(p->staging, [&](Staging& s) {
            if (cost) dc = s.take_out(cost, nT);
            if (lx) dl = s.take_out(lx, n_lx);
            if (lxx) dm = s.take_out(lxx, n_lxx);
        })) return 1;
    {
        ProfScope ps(c, ILQR_PROF_OTHER);
        launch_obs_derivs_any(p->bufs, p->obs, p->B, p->T, p->dims.n_x, 1, c->stream);
    }
    {
        ProfScope ps(c, ILQR_PROF_OTHER);
        launch_obs_query(p->obs, p->B, p->Bp, p->T, dof, dc, dl, dm, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    prof_mark(c, -1);
    return dev ? 0 : stg.fetch();
}
extern "C" int ilqr_problem_obstacle_terms(ilqr_problem* p, double* cost, double* lx, double* lxx) { return obstacle_terms(p, cost, lx, lxx, false); }
extern "C" int ilqr_problem_obstacle_terms_dev(ilqr_problem* p, double* cost, double* lx, double* lxx) { return obstacle_terms(p, cost, lx, lxx, true); }
