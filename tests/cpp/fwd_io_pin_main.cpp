// The pin FwdPin::WgIo of plan_riccati (ilqr_planner_amd/csrc/ilqr_plan.hpp) and RiccatiPlan::fwd_io: k_forward_reg with its helper waves.  The pin
// selects Forward::WaveWg with fwd_io on the single-integrator systems at any batch size and changes nothing else; pins 1 - 3 never set fwd_io;
// AUTO sets it exactly where fwd_io_auto says, on an unsplit solve that takes Forward::WaveWg.  Host-only (g++); built and run by
// tests/test_fwd_io_pin_cpu.py.  n_simd = 1024 (MI355X: 256 CUs) throughout.
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

// everything of a plan but the forward kernel's form
static bool same_rest(const RiccatiPlan& a, const RiccatiPlan& b) {
    return a.n_alpha == b.n_alpha && a.init == b.init && a.init_al_update == b.init_al_update && a.sweep == b.sweep && a.si_lanes[0] == b.si_lanes[0] &&
           a.si_lanes[1] == b.si_lanes[1] && a.si_wg[0] == b.si_wg[0] && a.si_wg[1] == b.si_wg[1] && a.si_io[0] == b.si_io[0] && a.si_io[1] == b.si_io[1] &&
           a.si_prep[0] == b.si_prep[0] && a.si_prep[1] == b.si_prep[1] && a.apply == b.apply && a.al_update == b.al_update && a.fused == b.fused &&
           a.kd_sym == b.kd_sym && a.split == b.split && a.needs_ws == b.needs_ws && a.obs_dense == b.obs_dense;
}

int main() {
    static_assert((int)FwdPin::WgIo == 4, "pin value of include/ilqr_hip.h (ILQR_XC_FWD_WG_IO)");
    static_assert(!RiccatiPlan{}.fwd_io, "off by default");
    for (int kind : {0, 2}) {
        for (int al = 0; al < 2; al++) {
            for (int unif = 0; unif < 2; unif++) {
                for (int split : {0, 1, 2}) {
                    for (int B : {1, 5, 16, 17, 67, 256, 2048, 3072, 3073, 4096, 4097, 8192}) {
                        PlanIn in = si(kind, al != 0, B, unif != 0);
                        in.split = split;
                        const RiccatiPlan autop = plan_riccati(in);
                        where = "AUTO";
                        CHECK(autop.fwd_io == (autop.forward == Forward::WaveWg && !autop.split && fwd_io_auto(B)));
                        CHECK(!autop.fwd_lds);
                        PlanIn pin = in;
                        where = "pin 4 (wgio)";
                        pin.forward = FwdPin::WgIo;
                        const RiccatiPlan io = plan_riccati(pin);
                        CHECK(io.forward == Forward::WaveWg); CHECK(io.fwd_io); CHECK(!io.fwd_lds);
                        where = "pin 1 (wg)";
                        pin.forward = FwdPin::Wg;
                        const RiccatiPlan wg = plan_riccati(pin);
                        CHECK(wg.forward == Forward::WaveWg); CHECK(!wg.fwd_io); CHECK(!wg.fwd_lds);
                        CHECK(same_rest(io, wg));  // pin 4 is pin 1 but for the form
                        where = "pin 2 (dpp)";
                        pin.forward = FwdPin::Dpp;
                        CHECK(!plan_riccati(pin).fwd_io);
                        where = "pin 3 (wglds)";
                        pin.forward = FwdPin::WgLds;
                        CHECK(!plan_riccati(pin).fwd_io); CHECK(plan_riccati(pin).fwd_lds);
                        where = "rest of the plan";
                        CHECK(io.sweep == autop.sweep && io.fused == autop.fused && io.kd_sym == autop.kd_sym && io.apply == autop.apply);
                        CHECK(io.split == autop.split && io.init == autop.init && io.n_alpha == autop.n_alpha && io.al_update == autop.al_update);
                        CHECK(io.si_lanes[0] == autop.si_lanes[0] && io.si_lanes[1] == autop.si_lanes[1] && io.si_wg[0] == autop.si_wg[0] && io.si_io[0] == autop.si_io[0]);
                        CHECK(io.si_prep[0] == autop.si_prep[0] && io.init_al_update == autop.init_al_update && io.needs_ws == autop.needs_ws);
                    }
                }
            }
        }
    }
    {   // the committed AUTO range, on the launched batch of an unsplit solve
        where = "AUTO range";
        for (int B = 1; B <= 20000; B++) {
            const PlanIn in = si(0, true, B, true);
            const RiccatiPlan p = plan_riccati(in);
            CHECK(!p.split);
            CHECK(p.fwd_io == (p.forward == Forward::WaveWg && B >= FWD_IO_MIN_BATCH && B <= FWD_IO_MAX_BATCH));
            if (fails) break;
        }
    }
    {   // where the wave forward passes do not apply, the pin selects nothing
        where = "other systems";
        PlanIn in = si(1, false, 4096, true);  // PosOrnTime
        in.nd = 2; in.forward = FwdPin::WgIo;
        const RiccatiPlan p = plan_riccati(in);
        CHECK(p.forward == Forward::Mfma); CHECK(!p.fwd_io);
        PlanIn p2 = si(0, false, 4096, true);  // PosOrn-2: the linear forward pass
        p2.nd = 2; p2.forward = FwdPin::WgIo;
        CHECK(plan_riccati(p2).forward == Forward::Lin); CHECK(!plan_riccati(p2).fwd_io);
        PlanIn g = si(0, false, 4096, true);
        g.generic = true; g.forward = FwdPin::WgIo;
        CHECK(plan_riccati(g).forward == Forward::Generic); CHECK(!plan_riccati(g).fwd_io);
        PlanIn many = si(0, false, 4096, true);  // more than 16 step sizes: no cooperative forward pass
        many.alpha_floor = 1e-9; many.forward = FwdPin::WgIo;
        CHECK(plan_riccati(many).forward == Forward::Generic); CHECK(!plan_riccati(many).fwd_io);
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
