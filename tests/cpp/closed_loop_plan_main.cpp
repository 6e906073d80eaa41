// The decision table of plan_closed_loop (ilqr_planner_amd/csrc/ilqr_closed_loop_plan.hpp): which kernel a closed-loop rollout runs for a
// system and a number of samples per instance, the samples per wave and the staged steps under the LDS budget.  Host-only (g++); built and
// run by tests/test_closed_loop_plan_cpu.py.
#include <cstdio>
#include <initializer_list>

#include "ilqr_closed_loop_plan.hpp"

using namespace ilqr;

static int fails = 0;
#define CHECK(cond)                                                                                              \
    do {                                                                                                         \
        if (!(cond)) { std::printf("FAIL [kind %d nd %d S %d] line %d: %s\n", kind, nd, S, __LINE__, #cond); fails++; } \
    } while (0)

struct SysRow { int kind, nd, record; int depth[6]; };  // depth at S = 4, 8, 16, 17, 64, 65
// record = n_u * rowp(n_x) + n_x + n_u doubles; depth = min(8, 40 KiB / ((64 / ns) * (record | 1) * 8))
static const SysRow SYSTEMS[] = {
    {0, 1, 70, {4, 8, 8, 8, 8, 8}},    // PosOrn-1:      16 x 568 B a step -> 4
    {0, 2, 133, {2, 4, 8, 8, 8, 8}},   // PosOrn-2:      16 x 1064 B -> 2, 8 x -> 4
    {1, 1, 96, {3, 6, 8, 8, 8, 8}},    // PosOrnTime-1:  16 x 776 B -> 3, 8 x -> 6
    {1, 2, 151, {2, 4, 8, 8, 8, 8}},   // PosOrnTime-2:  16 x 1208 B -> 2, 8 x -> 4
    {2, 1, 70, {4, 8, 8, 8, 8, 8}},    // JointSpace
    {3, 1, 96, {3, 6, 8, 8, 8, 8}},    // JointSpaceTime
};
static const int SAMPLES[] = {1, 3, 4, 8, 16, 17, 64, 65};
static const int NS[] = {0, 0, 4, 8, 16, 32, 64, 64};

int main() {
    for (const SysRow& r : SYSTEMS) {
        const int kind = r.kind, nd = r.nd;
        for (int i = 0; i < 8; i++) {
            const int S = SAMPLES[i];
            CHECK(cl_record(kind, nd) == r.record);
            CHECK(cl_stride(kind, nd) % 2 == 1 && cl_stride(kind, nd) >= cl_record(kind, nd));
            for (int B : {1, 13, 256, 4096}) {
                const ClosedLoopPlan p = plan_closed_loop(kind, nd, S, B, 1024, false);
                CHECK(p.coop == (S >= 4));   // fewer than 4 samples: the generic kernel
                if (p.coop) {
                    CHECK(p.ns == NS[i]);
                    CHECK(p.ns >= (S < 64 ? S : 64) && 64 % p.ns == 0);   // the group holds the samples (or a whole wave of them)
                    CHECK(p.depth == r.depth[i - 2]);
                    CHECK(p.depth >= CL_MIN_DEPTH && p.depth <= CL_MAX_DEPTH);
                    CHECK(p.lds_bytes == p.depth * (64 / p.ns) * cl_stride(kind, nd) * 8);
                    CHECK(p.lds_bytes <= CL_LDS_BUDGET);                  // the budget is never exceeded
                } else {
                    CHECK(p.ns == 0 && p.depth == 0 && p.lds_bytes == 0);
                }
                const ClosedLoopPlan g = plan_closed_loop(kind, nd, S, B, 1024, true);   // the generic pin is obeyed
                CHECK(!g.coop && g.lds_bytes == 0);
            }
        }
    }
    {   // every S up to 200: the budget holds and a wave's samples cover S with whole groups
        for (const SysRow& r : SYSTEMS) {
            const int kind = r.kind, nd = r.nd;
            for (int S = 1; S <= 200; S++) {
                const ClosedLoopPlan p = plan_closed_loop(kind, nd, S, 13, 1024, false);
                CHECK(p.lds_bytes <= CL_LDS_BUDGET);
                CHECK(!p.coop || (p.ns >= 4 && p.ns <= 64 && (p.ns & (p.ns - 1)) == 0 && (p.ns >= S || p.ns == 64)));
            }
        }
    }
    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
