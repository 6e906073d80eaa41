// ilqr_closed_loop_plan.hpp -- which kernel runs a batched closed-loop rollout (ilqr_problem_closed_loop): one pure decision from the system,
// the number of samples per instance and the context's pin, consumed by closed_loop (ilqr_capi_closed_loop.cpp).  No HIP here:
// tests/cpp/closed_loop_plan_main.cpp checks the table on the host.
#pragma once

namespace ilqr {

// LDS a workgroup (one wave) of k_closed_loop_coop may use.  A CU has 160 KiB and four SIMDs: 40 KiB leaves room for one wave per SIMD.
constexpr int CL_LDS_BUDGET = 40 * 1024;
constexpr int CL_MIN_SAMPLES = 4;   // fewer samples per instance: a wave would hold more than 16 instances' records and little is shared
constexpr int CL_MIN_DEPTH = 2;     // steps staged per block, at least / at most
constexpr int CL_MAX_DEPTH = 8;

// device dimensions (7 joints) of system (kind, nd): kind 0 PosOrn, 1 PosOrnTime, 2 JointSpace, 3 JointSpaceTime
constexpr int cl_nx(int kind, int nd) { return ((kind == 2 || kind == 3) ? 1 : nd) * 7 + ((kind == 1 || kind == 3) ? 1 : 0); }
constexpr int cl_nu(int kind) { return 7 + ((kind == 1 || kind == 3) ? 1 : 0); }
// doubles of one staged (instance, step) record: the plain gain record n_u x rowp (K_k | d_k | pad; the packed symmetric one is shorter and takes
// the same slot), xbar_k, ubar_k -- and its stride in LDS, made odd: the lanes of different instances then read different banks, the lanes of
// one instance the same address (a broadcast)
constexpr int cl_record(int kind, int nd) { return cl_nu(kind) * ((cl_nx(kind, nd) + 2) & ~1) + cl_nx(kind, nd) + cl_nu(kind); }
constexpr int cl_stride(int kind, int nd) { return cl_record(kind, nd) | 1; }

struct ClosedLoopPlan {
    bool coop = false;   // k_closed_loop_coop + k_closed_loop_kp; otherwise the generic k_closed_loop
    int ns = 0;          // samples of one instance in a wave (a power of two, 4 .. 64); the wave holds 64 / ns instances
    int depth = 0;       // steps whose records are staged in LDS at a time
    int lds_bytes = 0;   // depth * (64 / ns) * cl_stride * 8
};

// B and n_simd are part of the decision's interface for a crossover by launch size; none has been measured yet, so they do not enter it.
inline ClosedLoopPlan plan_closed_loop(int kind, int nd, int S, int B, int n_simd, bool generic_pin) {
    ClosedLoopPlan p;
    (void)B; (void)n_simd;
    if (generic_pin || S < CL_MIN_SAMPLES) return p;
    int ns = 4;
    while (ns < S && ns < 64) ns *= 2;   // the group that holds S, or 64 (further samples go to further waves)
    const int inst_step = cl_stride(kind, nd) * 8;
    while (ns < 64 && CL_LDS_BUDGET / ((64 / ns) * inst_step) < CL_MIN_DEPTH) ns *= 2;   // fewer instances per wave until two steps fit
    int depth = CL_LDS_BUDGET / ((64 / ns) * inst_step);
    if (depth < CL_MIN_DEPTH) return p;
    if (depth > CL_MAX_DEPTH) depth = CL_MAX_DEPTH;
    p.coop = true; p.ns = ns; p.depth = depth; p.lds_bytes = depth * (64 / ns) * inst_step;
    return p;
}

// Which kernel propagates the closed-loop covariance (ilqr_problem_closed_loop_cov, ilqr_closed_loop_cov.hpp).  Chains of fewer than 7 joints
// (the caller passes them as generic_pin, as for plan_closed_loop) and the generic pin take k_cl_cov, one lane per instance; everything else
// k_cl_cov_rows, 16 lanes per instance.  The two sum in different orders: they agree to rounding, not bit for bit.
struct ClosedLoopCovPlan {
    bool rows = false;   // k_cl_cov_rows; otherwise the generic k_cl_cov
};

// B and n_simd are part of the interface for a crossover by launch size; none has been measured, so they do not enter the decision.
inline ClosedLoopCovPlan plan_closed_loop_cov(int kind, int nd, int B, int n_simd, bool generic_pin) {
    ClosedLoopCovPlan p;
    (void)B; (void)n_simd;
    p.rows = !generic_pin && cl_nx(kind, nd) <= 15;
    return p;
}

// The refusals of ilqr_problem_closed_loop_cov that depend on the call's sizes alone: the error text, or null where the call is within both
// bounds.  n_x: the user's.  Pure, so that the bounds are checked without a problem of 2^31 entries (tests/cpp/closed_loop_cov_plan_main.cpp).
inline const char* cl_cov_size_refusal(long long B, long long T, long long n_kp, long long n_x, bool want_Sigma, bool want_kp_Sigma) {
    const long long lim = 1ll << 31;
    if (want_Sigma && B * T * n_x * n_x >= lim) return "closed loop cov: B * T * n_x^2 reaches 2^31 (ask for kp_Sigma, or split the batch)";
    if (want_kp_Sigma && B * n_kp * n_x * n_x >= lim) return "closed loop cov: B * n_kp * n_x^2 reaches 2^31 (split the batch)";
    return nullptr;
}

}  // namespace ilqr
