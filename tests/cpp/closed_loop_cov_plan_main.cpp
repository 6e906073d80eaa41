// The decision table of plan_closed_loop_cov (ilqr_planner_amd/csrc/ilqr_closed_loop_plan.hpp): which kernel propagates the closed-loop
// covariance for a system, and cl_cov_size_refusal, the two 32-bit bounds of the call with their error texts.  Host-only (g++); built and
// run by tests/test_closed_loop_cov_plan_cpu.py.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "ilqr_closed_loop_plan.hpp"

using namespace ilqr;

static int fails = 0;
#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) { std::printf("FAIL [kind %d nd %d B %d] line %d: %s\n", kind, nd, B, __LINE__, #cond); fails++; } \
    } while (0)

struct SysRow { int kind, nd, nx; };
static const SysRow SYSTEMS[] = {
    {0, 1, 7},    // PosOrn-1
    {0, 2, 14},   // PosOrn-2
    {1, 1, 8},    // PosOrnTime-1
    {1, 2, 15},   // PosOrnTime-2
    {2, 1, 7},    // JointSpace
    {3, 1, 8},    // JointSpaceTime
};

int main() {
    for (const SysRow& r : SYSTEMS) {
        const int kind = r.kind, nd = r.nd;
        for (int B : {1, 3, 4, 13, 256, 4096, 1 << 20}) {
            CHECK(cl_nx(kind, nd) == r.nx && r.nx <= 15);   // a row of Sigma per lane of a 16-lane DPP row
            for (int n_simd : {1, 1024}) {
                // every 7-joint system takes the row kernel at every batch size: no crossover has been measured
                CHECK(plan_closed_loop_cov(kind, nd, B, n_simd, false).rows);
                // the generic pin -- which is also how the caller routes a chain of fewer than 7 joints -- is obeyed
                CHECK(!plan_closed_loop_cov(kind, nd, B, n_simd, true).rows);
            }
        }
    }
    {   // the bounds: B T n_x^2 < 2^31 where Sigma is asked for, B n_kp n_x^2 < 2^31 where kp_Sigma is; each on its last legal and first refused B
        const int kind = -1, nd = -1, B = 0;   // (what CHECK prints)
        const long long lim = 1ll << 31;
        struct Case { long long T, n_kp, n_x; };
        for (const Case& q : {Case{25, 2, 15}, Case{2, 8, 15}, Case{200, 1, 7}, Case{9, 2, 3}, Case{100000, 8, 14}}) {
            const long long BS = (lim - 1) / (q.T * q.n_x * q.n_x), BK = (lim - 1) / (q.n_kp * q.n_x * q.n_x);   // the largest legal B of each bound
            CHECK(BS * q.T * q.n_x * q.n_x < lim && (BS + 1) * q.T * q.n_x * q.n_x >= lim);
            CHECK(cl_cov_size_refusal(BS, q.T, q.n_kp, q.n_x, true, false) == nullptr);
            const char* s = cl_cov_size_refusal(BS + 1, q.T, q.n_kp, q.n_x, true, false);
            CHECK(s && std::strstr(s, "B * T * n_x^2 reaches 2^31"));
            CHECK(cl_cov_size_refusal(BS + 1, q.T, q.n_kp, q.n_x, false, false) == nullptr);   // not asked for: no bound
            CHECK(cl_cov_size_refusal(BK, q.T, q.n_kp, q.n_x, false, true) == nullptr);
            const char* k = cl_cov_size_refusal(BK + 1, q.T, q.n_kp, q.n_x, false, true);
            CHECK(k && std::strstr(k, "B * n_kp * n_x^2 reaches 2^31"));
            CHECK(cl_cov_size_refusal(BK + 1, q.T, q.n_kp, q.n_x, false, false) == nullptr);
            if (q.T > q.n_kp) CHECK(cl_cov_size_refusal(BS + 1, q.T, q.n_kp, q.n_x, false, true) == nullptr);   // each output has its own bound
            CHECK(cl_cov_size_refusal(BK + 1, q.T, 0, q.n_x, false, true) == nullptr);                          // no keypoints: nothing to bound
        }
        // far beyond: no overflow of the products (B up to 2^31 - 1, T 10^5, n_x 15 stay below 2^63)
        CHECK(cl_cov_size_refusal(lim - 1, 100000, 8, 15, true, true) != nullptr);
    }
    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
