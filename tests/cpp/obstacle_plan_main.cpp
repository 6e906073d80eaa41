// plan_riccati (ilqr_planner_amd/csrc/ilqr_plan.hpp) with PlanIn::obstacles: a problem with obstacle terms runs on the generic kernel set --
// init, sweep and forward -- under every pin, exactly as the generic pin plans it; the flag is off by default, and with it off every shape of this
// grid is planned as it is without the field (the table itself: tests/cpp/plan_table_main.cpp).  Host-only (g++); built and run by
// tests/test_obstacle_plan_cpu.py.
#include <cstdio>
#include <initializer_list>

#include "ilqr_plan.hpp"

using namespace ilqr;

static int fails = 0;
#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        if (!(cond)) { std::printf("FAIL line %d: %s (kind %d nd %d al %d B %d)\n", __LINE__, #cond, kind, nd, al, B); fails++; } \
    } while (0)

static bool same(const RiccatiPlan& a, const RiccatiPlan& b) {
    bool s = a.n_alpha == b.n_alpha && a.init == b.init && a.init_al_update == b.init_al_update && a.sweep == b.sweep && a.forward == b.forward &&
             a.fwd_lds == b.fwd_lds && a.apply == b.apply && a.al_update == b.al_update && a.fused == b.fused && a.kd_sym == b.kd_sym &&
             a.split == b.split && a.needs_ws == b.needs_ws;
    for (int h = 0; h < 2; h++)
        s = s && a.si_lanes[h] == b.si_lanes[h] && a.si_wg[h] == b.si_wg[h] && a.si_io[h] == b.si_io[h] && a.si_prep[h] == b.si_prep[h];
    return s;
}

int main() {
    int n = 0;
    {
        const int kind = 0, nd = 1, al = 0, B = 0;
        CHECK(!PlanIn().obstacles);
    }
    for (int kind = 0; kind < 4; kind++)
        for (int nd = 1; nd <= (kind < 2 ? 2 : 1); nd++)
            for (int al = 0; al < 2; al++)
                for (int B : {1, 256, 2048, 4096, 10000})
                    for (int nb_iter : {0, 10})
                        for (int split : {0, 1, 2})
                            for (SweepPin sw : {SweepPin::Auto, SweepPin::Mfma, SweepPin::Rows, SweepPin::SiWave, SweepPin::SiWg, SweepPin::SiWgIo, SweepPin::SiWgPrep})
                                for (FwdPin fw : {FwdPin::Auto, FwdPin::Wg, FwdPin::Dpp, FwdPin::WgLds})
                                    for (RerollPin rr : {RerollPin::Auto, RerollPin::Rows, RerollPin::Dpp}) {
                                        PlanIn in;
                                        in.kind = kind; in.nd = nd; in.al = al != 0; in.B = B; in.n_simd = 1024; in.halves = B >= SPLIT_MIN_BATCH;
                                        in.nb_iter = nb_iter; in.uniform_R = true; in.split = split;
                                        if (al) { in.m = 2; in.con_state_only = true; }
                                        in.sweep = sw; in.forward = fw; in.reroll = rr;
                                        const RiccatiPlan off = plan_riccati(in);
                                        PlanIn g = in;
                                        g.generic = true;
                                        const RiccatiPlan pinned = plan_riccati(g);
                                        in.obstacles = true;
                                        const RiccatiPlan p = plan_riccati(in);
                                        CHECK(p.init == Init::Generic); CHECK(p.sweep == Sweep::Generic); CHECK(p.forward == Forward::Generic);
                                        CHECK(p.apply == Apply::None); CHECK(!p.split); CHECK(!p.fused); CHECK(!p.al_update); CHECK(!p.init_al_update);
                                        CHECK(p.needs_ws == (nb_iter > 0)); CHECK(p.kd_sym == (nb_iter > 0 ? 0 : KD_SYM_KEEP));
                                        CHECK(same(p, pinned));
                                        in.generic = true;   // the pin on top changes nothing
                                        CHECK(same(plan_riccati(in), p));
                                        in.generic = false; in.obstacles = false;
                                        CHECK(same(plan_riccati(in), off));
                                        if (B >= 256 && !al) CHECK(off.sweep != Sweep::Generic);   // the grid does hold cooperative plans to lose
                                        n++;
                                    }
    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("%d plans\nok\n", n);
    return 0;
}
