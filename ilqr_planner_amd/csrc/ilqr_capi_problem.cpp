// ilqr_capi_problem.cpp -- C ABI (include/ilqr_hip.h): lowering of the POD problem description to the device descriptor, problem creation and
// destruction, the setters, the constraints and stand-alone FK.
#include "ilqr_capi_internal.hpp"

using namespace ilqr_capi;

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
int ilqr_capi::lower_chain(ilqr_ctx* c, const ilqr_problem_desc& d, DevChain& ch) {
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
    for (DevScratch* b : {&p->staging, &p->cl_kpx, &p->cl_rep, &p->cl_con_ws, &p->cl_cost, &p->cl_cov_ws, &p->cl_cov_kps}) b->release();
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
    Staging stg{c};
    if (!src_is_dev && stg.lay(p->staging, [&](Staging& s) { dsrc = s.take_in(src, n); })) return 1;
    if (m) launch_to_soa_map(dsrc, dst, p->B, p->Bp, outer, *m, c->stream);
    else launch_to_soa(dsrc, dst, p->B, p->Bp, rows, c->stream);
    HIPCHK(c, hipGetLastError());
    return src_is_dev ? 0 : stg.fetch();  // waits: staging is reused; the host buffer may go away
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
    struct Local : DevScratch { ~Local() { release(); } } buf;  // this call's own staging, freed on every way out
    const DevDesc* dd = nullptr;
    const double* dq = nullptr;
    double *dp = nullptr, *dqt = nullptr, *dj = nullptr;
    Staging stg{c};
    if (stg.lay(buf, [&](Staging& s) {
            dd = s.take_in(&h, 1);
            dq = s.take_in(q, (size_t)n * DOF);
            if (pos) dp = s.take_out(pos, (size_t)n * 3);
            if (quat) dqt = s.take_out(quat, (size_t)n * 4);
            if (jac) dj = s.take_out(jac, (size_t)n * 6 * DOF);
        })) return 1;
    launch_fk_batch(dd, n, dq, dp, dqt, dj, c->stream);
    HIPCHK(c, hipGetLastError());
    if (stg.fetch()) return 1;
    if (jac && dof != DOF)
        for (size_t r = 0; r < (size_t)n * 6; r++) std::memcpy(jac_out + r * dof, &jw[r * DOF], sizeof(double) * dof);
    return 0;
}
