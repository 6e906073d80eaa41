// plan_riccati (ilqr_planner_amd/csrc/ilqr_plan.hpp) with PlanIn::obstacles_coop, over the grid of tests/cpp/obstacle_plan_main.cpp: with the flag
// off every plan is the plan of the input without the field; with obstacles && obstacles_coop the single-integrator shapes get the dense
// cooperative plan (LTI init, the register-resident sweep not fused on lone waves, a wave forward pass, k_apply every iteration, no split) and
// every other shape the plan of the flag off; the flag without obstacles changes nothing.  Host-only (g++); built and run by
// tests/test_obstacle_coop_plan_cpu.py.
#include <cstdio>
#include <initializer_list>

#include "ilqr_plan.hpp"

using namespace ilqr;

static int fails = 0;
#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        if (!(cond)) { std::printf("FAIL line %d: %s (kind %d nd %d al %d B %d)\n", __LINE__, #cond, in.kind, in.nd, (int)in.al, in.B); fails++; } \
    } while (0)

static bool same(const RiccatiPlan& a, const RiccatiPlan& b) {
    bool s = a.n_alpha == b.n_alpha && a.init == b.init && a.init_al_update == b.init_al_update && a.sweep == b.sweep && a.forward == b.forward &&
             a.fwd_lds == b.fwd_lds && a.apply == b.apply && a.al_update == b.al_update && a.fused == b.fused && a.kd_sym == b.kd_sym &&
             a.split == b.split && a.needs_ws == b.needs_ws && a.obs_dense == b.obs_dense;
    for (int h = 0; h < 2; h++)
        s = s && a.si_lanes[h] == b.si_lanes[h] && a.si_wg[h] == b.si_wg[h] && a.si_io[h] == b.si_io[h] && a.si_prep[h] == b.si_prep[h];
    return s;
}

// the plan of section "The plan" for an eligible input
static void check_dense(const PlanIn& in) {
    const RiccatiPlan p = plan_riccati(in);
    CHECK(p.obs_dense);
    CHECK(p.init == Init::Lti); CHECK(p.init_al_update == in.al);
    CHECK(p.sweep == Sweep::SiDpp); CHECK(!p.fused);
    CHECK(p.si_lanes[0] == ((in.B + 3) / 4 <= in.n_simd ? 16 : 8));
    for (int h = 0; h < 2; h++) { CHECK(!p.si_wg[h]); CHECK(!p.si_io[h]); CHECK(!p.si_prep[h]); }
    const bool dpp = in.forward == FwdPin::Dpp || (in.forward == FwdPin::Auto && (in.B + 3) / 4 <= 3 * in.n_simd / 4);
    CHECK(p.forward == (dpp ? Forward::WaveDpp : Forward::WaveWg));
    CHECK(p.fwd_lds == (in.forward == FwdPin::WgLds));
    CHECK(p.apply == Apply::Wave); CHECK(!p.al_update);
    CHECK(p.kd_sym == (in.nb_iter == 0 ? KD_SYM_KEEP : 0));
    CHECK(!p.split); CHECK(!p.needs_ws);
    CHECK(p.n_alpha == n_alpha_of(in.line_search, in.alpha_floor));
}
// not eligible: field by field the plan with the flag off
static void check_as_off(PlanIn in) {
    const RiccatiPlan p = plan_riccati(in);
    CHECK(!p.obs_dense);
    in.obstacles_coop = false;
    CHECK(same(p, plan_riccati(in)));
}

int main() {
    int n = 0, dense = 0;
    {
        PlanIn in;
        CHECK(!in.obstacles_coop);
        CHECK(!RiccatiPlan().obs_dense);
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
                                        CHECK(!off.obs_dense);
                                        in.obstacles_coop = true;   // without obstacles: nothing
                                        CHECK(same(plan_riccati(in), off));
                                        in.obstacles = true;
                                        const bool single = (kind == 0 || kind == 2) && nd == 1;
                                        if (single) { check_dense(in); dense++; }
                                        else check_as_off(in);
                                        PlanIn g = in;
                                        g.generic = true;   // the generic pin wins over the mode
                                        check_as_off(g);
                                        CHECK(plan_riccati(g).sweep == Sweep::Generic);
                                        if (single) {   // every reason to stay on today's plan
                                            PlanIn q = in; q.limits2_set = true; check_as_off(q);
                                            q = in; q.shared_steps = true; check_as_off(q);
                                            q = in; q.off32 = false; check_as_off(q);
                                            q = in; q.alpha_floor = 1e-5; CHECK(n_alpha_of(true, q.alpha_floor) == 18); check_as_off(q);
                                            q = in; q.alpha_floor = 2e-5; CHECK(n_alpha_of(true, q.alpha_floor) == 17); check_as_off(q);
                                            q = in; q.alpha_floor = 4e-5; CHECK(n_alpha_of(true, q.alpha_floor) == 16); check_dense(q);
                                            if (al) {
                                                q = in; q.m = 5; check_as_off(q);
                                                q = in; q.m = 4; check_dense(q);
                                                q = in; q.m = 1; check_dense(q);
                                                q = in; q.per_step = 1; check_as_off(q);
                                                q = in; q.con_state_only = false; check_as_off(q);
                                            }
                                            q = in; q.uniform_R = false; check_dense(q);
                                            q = in; q.line_search = false; check_dense(q);
                                            q = in; q.profile = true; check_dense(q);
                                        }
                                        n++;
                                    }
    // both lane groupings around B = 4 n_simd, the forward choice around 3 n_simd, on two machine sizes
    for (int n_simd : {1024, 416})
        for (int al = 0; al < 2; al++) {
            PlanIn in;
            in.kind = 0; in.nd = 1; in.al = al != 0; in.n_simd = n_simd; in.nb_iter = 5; in.obstacles = in.obstacles_coop = true;
            if (al) { in.m = 1; in.con_state_only = true; }
            in.B = 4 * n_simd; in.halves = true;
            check_dense(in); CHECK(plan_riccati(in).si_lanes[0] == 16);
            in.B = 4 * n_simd + 1;
            check_dense(in); CHECK(plan_riccati(in).si_lanes[0] == 8);
            in.B = 3 * n_simd;
            check_dense(in); CHECK(plan_riccati(in).forward == Forward::WaveDpp);
            in.B = 3 * n_simd + 1;
            check_dense(in); CHECK(plan_riccati(in).forward == Forward::WaveWg);
            in.forward = FwdPin::Dpp;
            check_dense(in); CHECK(plan_riccati(in).forward == Forward::WaveDpp);
            in.B = 16; in.forward = FwdPin::Wg;
            check_dense(in); CHECK(plan_riccati(in).forward == Forward::WaveWg && !plan_riccati(in).fwd_lds);
            in.forward = FwdPin::WgLds;
            check_dense(in); CHECK(plan_riccati(in).forward == Forward::WaveWg && plan_riccati(in).fwd_lds);
        }
    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("%d plans, %d of them dense\nok\n", n, dense);
    return 0;
}
