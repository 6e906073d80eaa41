// ilqr_rollout_kernels.hpp -- the two sequential rollout kernels of the generic (lane-per-instance) set, k_init_rollout and k_forward, as
// templates in a header: ilqr_kernels.hip instantiates the forms without obstacle terms and the ObsArgs forms, and the unit built with
// ilqr_capi_kernels.cpp (ilqr_obstacle_coop_kernels.hpp) the ObsSelfArgs forms of a geometry with self pairs -- so that ilqr_kernels.hip's code object
// holds what it held before there were self pairs.  Included inside namespace ilqr, behind ilqr_step.hpp and an overload
// obs_stage_cost(O, b, x) for every O the unit instantiates.
#pragma once

// Initial rollout from U0 (ILQRRecursive.cpp:27-56): X, cost0; resets the per-instance solve state.
// O is empty, or ObsArgs: the OBS form, in which the obstacle term of every state joins its stage cost.  (A trailing pack and not a flag with an
// argument, here and in k_backward / k_forward: the forms without the terms keep their text, their arguments and their code.)
template <class S, bool AL, class... O>
__global__ __launch_bounds__(64) void k_init_rollout(Bufs a, double penalty, O... o) {
    constexpr int NX = S::NX, NU = S::NU;
    constexpr bool OBS = sizeof...(O) != 0;
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= d.B) return;
    const int Bp = d.Bp, T = d.T;
    double x[NX], u[NU], xn[NX];
    init_state<S>(d, a, b, x);
    double cost = 0;
    int st = 0;  // next entry of the step table (ilqr_steps.hpp): all keypoints on one timestep add their terms
    double* X = a.X[0];
    double* U = a.U[0];
    for (int k = 0; k < T - 1; k++) {
        UNR for (int i = 0; i < NX; i++) AT(X, k * NX + i, b) = x[i];
        UNR for (int i = 0; i < NU; i++) { u[i] = AT(a.U0, k * NU + i, b); AT(U, k * NU + i, b) = u[i]; }
        if (AL) {
            for (int r = 0; r < a.m; r++) {
                double g = con_g<S>(a, k, r, x, u);
                double lam = AT(a.lambda, k * a.m + r, b);
                AT(a.Is, k * a.m + r, b) = penalty * ((g < 0 && lam == 0) ? 0.0 : 1.0);
            }
        }
        const bool iskp = (st < d.steps.n && d.steps.t[st] == k);
        if constexpr (OBS) cost += stage_cost<S>(d, a, b, iskp ? st : -1, x, u) + obs_stage_cost(o..., b, x);
        else cost += stage_cost<S>(d, a, b, iskp ? st : -1, x, u);
        if (iskp) st++;
        dyn_step<S>(d, x, u, xn);
        UNR for (int i = 0; i < NX; i++) x[i] = xn[i];
    }
    UNR for (int i = 0; i < NX; i++) AT(X, (T - 1) * NX + i, b) = x[i];
    {
        const bool iskp = (st < d.steps.n && d.steps.t[st] == T - 1);
        double zu[NU];
        UNR for (int i = 0; i < NU; i++) zu[i] = 0;
        if constexpr (OBS) cost += stage_cost<S>(d, a, b, iskp ? st : -1, x, zu) + obs_stage_cost(o..., b, x);
        else cost += stage_cost<S>(d, a, b, iskp ? st : -1, x, zu);
    }
    a.cost[b] = cost;
    a.alpha[b] = 1.0;
    a.cur[b] = 0;
    a.active[b] = 1;
    a.iters[b] = 0;
    a.pend[b] = 0;
    a.pred[b] = 0;
    a.status[b] = isfinite(cost) ? 0 : 1;
}

// Forward pass with step-halving line search (ILQRRecursive.cpp:101-176).  Each trial re-rolls the whole horizon
// and overwrites the instance's inactive trajectory buffer; the last trial executed is the accepted one.
// O = ObsArgs, the OBS form: the obstacle term of every state joins its stage cost, as in k_init_rollout.
template <class S, bool AL, class... O>
__global__ __launch_bounds__(64) void k_forward(Bufs a, int it, int line_search, int early_stop, double penalty_roll,
                                                double penalty_update, int do_update, int nb_iter, O... o) {
    constexpr int NX = S::NX, NU = S::NU;
    constexpr bool OBS = sizeof...(O) != 0;
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= d.B) return;
    if (!a.active[b]) return;
    const int Bp = d.Bp, T = d.T;
    const int cur = a.cur[b];
    const double* X = a.X[cur];
    const double* U = a.U[cur];
    double* Xn = a.X[1 - cur];
    double* Un = a.U[1 - cur];
    const double cost0 = a.cost[b];
    double alpha = 2, newCost = 0, dun = 0;
    do {
        alpha /= 2.0;
        double x[NX], xn[NX], u[NU];
        init_state<S>(d, a, b, x);
        dun = 0;
        newCost = 0;
        int st = 0;  // step table walk, as in k_init_rollout
        for (int k = 0; k < T - 1; k++) {
            double dx[NX];
            UNR for (int i = 0; i < NX; i++) dx[i] = x[i] - AT(X, k * NX + i, b);
            double n2 = 0;
            UNR for (int i = 0; i < NU; i++) {
                double s = 0;
                UNR for (int j = 0; j < NX; j++) s += KD_REC(a.KD, Bp, NU * kd_rowp(NX), k, b)[i * kd_rowp(NX) + j] * dx[j];
                double du = s + alpha * KD_REC(a.KD, Bp, NU * kd_rowp(NX), k, b)[i * kd_rowp(NX) + NX];
                n2 += du * du;
                u[i] = AT(U, k * NU + i, b) + du;
            }
            dun += sqrt(n2);  // accumulates ||du||, not ||du||^2 (ILQRRecursive.cpp:132)
            UNR for (int i = 0; i < NX; i++) AT(Xn, k * NX + i, b) = x[i];
            UNR for (int i = 0; i < NU; i++) AT(Un, k * NU + i, b) = u[i];
            if (AL) {
                for (int r = 0; r < a.m; r++) {
                    double g = con_g<S>(a, k, r, x, u);
                    double lam = AT(a.lambda, k * a.m + r, b);
                    AT(a.Is, k * a.m + r, b) = penalty_roll * ((g < 0 && lam == 0) ? 0.0 : 1.0);
                }
            }
            const bool iskp = (st < d.steps.n && d.steps.t[st] == k);
            if constexpr (OBS) newCost += stage_cost<S>(d, a, b, iskp ? st : -1, x, u) + obs_stage_cost(o..., b, x);
            else newCost += stage_cost<S>(d, a, b, iskp ? st : -1, x, u);
            if (iskp) st++;
            dyn_step<S>(d, x, u, xn);
            UNR for (int i = 0; i < NX; i++) x[i] = xn[i];
        }
        UNR for (int i = 0; i < NX; i++) AT(Xn, (T - 1) * NX + i, b) = x[i];
        {
            const bool iskp = (st < d.steps.n && d.steps.t[st] == T - 1);
            double zu[NU];
            UNR for (int i = 0; i < NU; i++) zu[i] = 0;
            if constexpr (OBS) newCost += stage_cost<S>(d, a, b, iskp ? st : -1, x, zu) + obs_stage_cost(o..., b, x);
            else newCost += stage_cost<S>(d, a, b, iskp ? st : -1, x, zu);
        }
    } while (((newCost >= cost0) || isnan(newCost)) && alpha > d.alpha_floor && line_search);

    if (AL && do_update) {  // multiplier update with the UPDATED penalty, on the accepted trajectory (AL-ILQR.cpp:202-208)
        for (int k = 0; k < T - 1; k++) {
            double x[NX], u[NU];
            UNR for (int i = 0; i < NX; i++) x[i] = AT(Xn, k * NX + i, b);
            UNR for (int i = 0; i < NU; i++) u[i] = AT(Un, k * NU + i, b);
            for (int r = 0; r < a.m; r++) {
                double g = con_g<S>(a, k, r, x, u);
                double v = AT(a.lambda, k * a.m + r, b) + penalty_update * g;
                AT(a.lambda, k * a.m + r, b) = v > 0 ? v : 0;
            }
        }
    }
    // accept unconditionally (ILQRRecursive.cpp:157-162)
    a.cost[b] = newCost;
    a.alpha[b] = alpha;
    a.cur[b] = 1 - cur;
    a.iters[b] = it + 1;
    a.status[b] = (isfinite(newCost) ? 0 : 1) | ((alpha <= d.alpha_floor) ? 2 : 0);
    if (a.cost_trace) {
        a.cost_trace[(size_t)it * Bp + b] = newCost;
        a.alpha_trace[(size_t)it * Bp + b] = alpha;
    }
    bool stop = early_stop && (alpha * sqrt(dun) < d.stop_tol);
    if (!AL) stop = stop && (newCost < 1e-3);  // ILQRRecursive.cpp:174 vs AL-ILQR.cpp:225
    if (stop) a.active[b] = 0;
}
