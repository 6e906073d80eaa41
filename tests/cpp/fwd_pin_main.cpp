// The forward-pass pins of plan_riccati (ilqr_planner_amd/csrc/ilqr_plan.hpp) on the single-integrator systems: Forward::WaveWg is the large-batch
// forward pass, k_forward_reg by default and under FwdPin::Wg; FwdPin::WgLds selects its predecessor k_forward_wg (the bitwise reference) at any
// batch size.  Host-only (g++); built and run by tests/test_fwd_pin_cpu.py.  n_simd = 1024 (MI355X: 256 CUs) throughout.
#include <cstdio>
#include <initializer_list>

#include "ilqr_plan.hpp"

using namespace ilqr;

static int fails = 0;
static const char* where = "";
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { std::printf("FAIL [%s] line %d: %s\n", where, __LINE__, #cond); fails++; } \
    } while (0)

static PlanIn si(int kind, bool al, int B, bool uniform_R) {
    PlanIn in;
    in.kind = kind; in.nd = 1; in.al = al; in.B = B; in.n_simd = 1024; in.halves = B >= SPLIT_MIN_BATCH;
    in.nb_iter = 10; in.uniform_R = uniform_R;
    if (al) { in.m = 2; in.con_state_only = true; }
    return in;
}

int main() {
    static_assert((int)FwdPin::Auto == 0 && (int)FwdPin::Wg == 1 && (int)FwdPin::Dpp == 2 && (int)FwdPin::WgLds == 3, "pin values of include/ilqr_hip.h");
    for (int kind : {0, 2}) {
        for (int al = 0; al < 2; al++) {
            for (int unif = 0; unif < 2; unif++) {
                for (int B : {1, 5, 16, 17, 67, 256, 2048, 3072, 3073, 4096, 4097, 8192}) {
                    const PlanIn in = si(kind, al != 0, B, unif != 0);
                    const RiccatiPlan autop = plan_riccati(in);
                    where = "AUTO";
                    CHECK(autop.forward == (B > 3072 ? Forward::WaveWg : Forward::WaveDpp));
                    CHECK(!autop.fwd_lds);  // AUTO never runs the old kernel
                    PlanIn pin = in;
                    where = "pin 1 (wg)";
                    pin.forward = FwdPin::Wg;
                    const RiccatiPlan wg = plan_riccati(pin);
                    CHECK(wg.forward == Forward::WaveWg); CHECK(!wg.fwd_lds);
                    where = "pin 3 (wglds)";
                    pin.forward = FwdPin::WgLds;
                    const RiccatiPlan lds = plan_riccati(pin);
                    CHECK(lds.forward == Forward::WaveWg); CHECK(lds.fwd_lds);
                    where = "pin 2 (dpp)";
                    pin.forward = FwdPin::Dpp;
                    const RiccatiPlan dpp = plan_riccati(pin);
                    CHECK(dpp.forward == Forward::WaveDpp); CHECK(!dpp.fwd_lds);
                    // the pin changes the forward kernel and nothing else: same sweep, record layout, apply pass, split
                    where = "rest of the plan";
                    for (const RiccatiPlan* q : {&wg, &lds, &dpp}) {
                        CHECK(q->sweep == autop.sweep && q->fused == autop.fused && q->kd_sym == autop.kd_sym && q->apply == autop.apply);
                        CHECK(q->split == autop.split && q->init == autop.init && q->n_alpha == autop.n_alpha && q->al_update == autop.al_update);
                        CHECK(q->si_lanes[0] == autop.si_lanes[0] && q->si_lanes[1] == autop.si_lanes[1]);
                    }
                }
            }
        }
    }
    {   // where the wave forward passes do not apply, the pin selects nothing
        where = "other systems";
        PlanIn in = si(1, false, 4096, true);  // PosOrnTime
        in.nd = 2; in.forward = FwdPin::WgLds;
        const RiccatiPlan p = plan_riccati(in);
        CHECK(p.forward == Forward::Mfma); CHECK(!p.fwd_lds);
        PlanIn g = si(0, false, 4096, true);
        g.generic = true; g.forward = FwdPin::WgLds;
        CHECK(plan_riccati(g).forward == Forward::Generic); CHECK(!plan_riccati(g).fwd_lds);
        PlanIn many = si(0, false, 4096, true);  // more than 16 step sizes: no cooperative forward pass
        many.alpha_floor = 1e-9; many.forward = FwdPin::WgLds;
        CHECK(plan_riccati(many).forward == Forward::Generic); CHECK(!plan_riccati(many).fwd_lds);
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
