// The sweep pins SweepPin::SiWave / SweepPin::SiWg of plan_riccati (ilqr_planner_amd/csrc/ilqr_plan.hpp): the form of k_backward_si_dpp -- lone waves or
// workgroups of four waves, the four that share every 128-byte line of x, u (same bits).  They are honoured only where the sweep is Sweep::SiDpp with 16
// lanes per instance, AUTO switches at SI_WG_MIN_BATCH launched instances, and neither they nor the new field change anything else of the plan.
// Host-only (g++); built and run by tests/test_sweep_pin_cpu.py.  n_simd = 1024 (MI355X: 256 CUs) throughout.
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "ilqr_plan.hpp"

using namespace ilqr;

static int fails = 0;
static const char* where = "";
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { std::printf("FAIL [%s] line %d: %s\n", where, __LINE__, #cond); fails++; } \
    } while (0)

// the inputs of tests/cpp/plan_table_main.cpp
static PlanIn base(int kind, int nd, bool al, int B) {
    PlanIn in;
    in.kind = kind; in.nd = nd; in.al = al; in.B = B; in.n_simd = 1024; in.halves = B >= SPLIT_MIN_BATCH;
    in.nb_iter = 10; in.uniform_R = true;
    return in;
}
static PlanIn c3(int B) {
    PlanIn in = base(0, 1, true, B);
    in.m = 2; in.con_state_only = true;
    return in;
}
static PlanIn c2(int B) { return base(0, 1, false, B); }
static PlanIn c4(int B) { return base(1, 2, false, B); }
static PlanIn with_control_row(PlanIn in, int m = 2) { in.m = m; in.con_state_only = false; return in; }
template <class F>
static PlanIn mod(PlanIn in, F f) { f(in); return in; }

static std::vector<PlanIn> table_inputs() {
    std::vector<PlanIn> v;
    for (int B : {256, 3072, 3073, 4096, 4097, 4100, 8192, 10000}) v.push_back(c3(B));
    for (int B : {256, 1024, 1025, 2048, 2049, 4096}) v.push_back(c4(B));
    v.push_back(c2(256));
    v.push_back(mod(c3(4096), [](PlanIn& i) { i.uniform_R = false; }));
    v.push_back(mod(c4(4096), [](PlanIn& i) { i.line_search = false; }));
    v.push_back(mod(c4(4096), [](PlanIn& i) { i.reroll = RerollPin::Dpp; }));
    v.push_back(mod(c3(256), [](PlanIn& i) { i.forward = FwdPin::Wg; }));
    v.push_back(mod(c3(4096), [](PlanIn& i) { i.forward = FwdPin::Dpp; }));
    for (int B : {256, 4096}) {
        v.push_back(with_control_row(base(1, 1, true, B), 17));
        v.push_back(with_control_row(base(0, 2, true, B), 16));
        v.push_back(with_control_row(c3(B)));
        v.push_back(with_control_row(base(2, 1, true, B)));
        for (int m : {4, 5}) {
            v.push_back(mod(c3(B), [m](PlanIn& i) { i.m = m; }));
            v.push_back(mod(base(2, 1, true, B), [m](PlanIn& i) { i.m = m; i.con_state_only = true; }));
        }
        for (int per_step = 0; per_step < 2; per_step++)
            for (int so = 0; so < 2; so++) {
                v.push_back(mod(c3(B), [=](PlanIn& i) { i.m = 4; i.per_step = per_step; i.con_state_only = so != 0; }));
                v.push_back(mod(base(2, 1, true, B), [=](PlanIn& i) { i.m = 4; i.per_step = per_step; i.con_state_only = so != 0; }));
            }
        for (int nd = 1; nd <= 2; nd++)
            for (int kind : {0, 1, 3}) {
                if (kind == 3 && nd == 2) continue;
                for (int m : {16, 17}) v.push_back(mod(base(kind, nd, true, B), [m](PlanIn& i) { i.m = m; i.con_state_only = true; }));
            }
    }
    for (int kind = 0; kind < 4; kind++) {
        v.push_back(mod(base(kind, kind == 1 ? 2 : 1, true, 4096), [](PlanIn& i) { i.m = 2; i.con_state_only = true; i.generic = true; }));
        v.push_back(mod(base(kind, kind == 1 ? 2 : 1, true, 4096), [](PlanIn& i) { i.m = 2; i.con_state_only = true; i.limits2_set = true; }));
    }
    v.push_back(mod(c3(4096), [](PlanIn& i) { i.alpha_floor = 1e-6; }));
    for (int B : {2048, 4096}) v.push_back(mod(c3(B), [](PlanIn& i) { i.off32 = false; }));
    for (PlanIn in : {c3(4096), c4(2048), with_control_row(base(2, 1, true, 256))}) v.push_back(mod(in, [](PlanIn& i) { i.nb_iter = 0; }));
    v.push_back(mod(c4(2048), [](PlanIn& i) { i.profile = true; }));
    v.push_back(mod(c4(2048), [](PlanIn& i) { i.split = 0; }));
    for (int B : {4096, 8192, 10000}) v.push_back(mod(c3(B), [](PlanIn& i) { i.split = 2; }));
    v.push_back(mod(with_control_row(base(2, 1, true, 4096)), [](PlanIn& i) { i.split = 2; }));
    return v;
}

// every field but si_wg
static bool same_but_form(const RiccatiPlan& a, const RiccatiPlan& b) {
    return a.n_alpha == b.n_alpha && a.init == b.init && a.init_al_update == b.init_al_update && a.sweep == b.sweep && a.si_lanes[0] == b.si_lanes[0] &&
           a.si_lanes[1] == b.si_lanes[1] && a.forward == b.forward && a.fwd_lds == b.fwd_lds && a.apply == b.apply && a.al_update == b.al_update &&
           a.fused == b.fused && a.kd_sym == b.kd_sym && a.split == b.split && a.needs_ws == b.needs_ws;
}

int main() {
    static_assert((int)SweepPin::Auto == 0 && (int)SweepPin::Mfma == 1 && (int)SweepPin::Rows == 2 && (int)SweepPin::SiWave == 4 && (int)SweepPin::SiWg == 5,
                  "pin values of include/ilqr_hip.h");
    static_assert(SI_WG_MIN_BATCH == 256, "the threshold documented in include/ilqr_hip.h and DESIGN.md 5.3");
    {   // the single-integrator sweep: C3, C2, JointSpace-1, any R
        for (int kind : {0, 2})
            for (int al = 0; al < 2; al++)
                for (int B : {1, 5, 16, 17, 67, 256, 1024, SI_WG_MIN_BATCH - 1, SI_WG_MIN_BATCH, 3072, 4096, 4097, 8192}) {
                    PlanIn in = base(kind, 1, al != 0, B);
                    if (al) { in.m = 2; in.con_state_only = true; }
                    const RiccatiPlan autop = plan_riccati(in);
                    where = "AUTO";
                    CHECK(autop.sweep == Sweep::SiDpp); CHECK(!autop.split);
                    CHECK(autop.si_lanes[0] == (B <= 4096 ? 16 : 8));
                    CHECK(autop.si_wg[0] == (B >= SI_WG_MIN_BATCH && B <= 4096));  // the 8-lane grouping stays on lone waves
                    where = "pin 4 (siwave)";
                    in.sweep = SweepPin::SiWave;
                    const RiccatiPlan wave = plan_riccati(in);
                    CHECK(!wave.si_wg[0]); CHECK(!wave.si_wg[1]);
                    where = "pin 5 (siwg)";
                    in.sweep = SweepPin::SiWg;
                    const RiccatiPlan wg = plan_riccati(in);
                    CHECK(wg.si_wg[0] == (B <= 4096));
                    where = "rest of the plan";
                    CHECK(same_but_form(wave, autop)); CHECK(same_but_form(wg, autop));
                    where = "pins mfma / rows";   // they select nothing on this sweep, as before
                    for (SweepPin pin : {SweepPin::Mfma, SweepPin::Rows}) {
                        in.sweep = pin;
                        const RiccatiPlan q = plan_riccati(in);
                        CHECK(same_but_form(q, autop)); CHECK(q.si_wg[0] == autop.si_wg[0]); CHECK(q.si_wg[1] == autop.si_wg[1]);
                    }
                }
    }
    {   // split halves: the form follows the launched half, as the lane count does
        where = "split 2";
        PlanIn in = c3(8192);
        in.split = 2;
        RiccatiPlan p = plan_riccati(in);   // two halves of 4096
        CHECK(p.split); CHECK(p.si_wg[0]); CHECK(p.si_wg[1]);
        in.sweep = SweepPin::SiWave;         // (a split half has at least SPLIT_MIN_BATCH / 2 instances: always above the threshold)
        p = plan_riccati(in);
        CHECK(p.split); CHECK(!p.si_wg[0]); CHECK(!p.si_wg[1]);
        in.sweep = SweepPin::SiWg;
        p = plan_riccati(in);
        CHECK(p.si_wg[0]); CHECK(p.si_wg[1]);
        static_assert(SI_WG_MIN_BATCH <= SPLIT_MIN_BATCH / 2, "");
        in = c3(10000);                      // 8 lanes per instance in both halves
        in.split = 2; in.sweep = SweepPin::SiWg;
        p = plan_riccati(in);
        CHECK(p.si_lanes[0] == 8); CHECK(!p.si_wg[0]); CHECK(!p.si_wg[1]);
    }
    // every input of the plan table: the two new pins act as AUTO wherever the sweep is not SiDpp, and change nothing but the form where it is;
    // Mfma / Rows keep their meaning (the AUTO plan of an unpinned input, the pinned plan itself otherwise, is what plan_table_main.cpp checks)
    for (const PlanIn& in0 : table_inputs()) {
        where = "plan table";
        const RiccatiPlan ref = plan_riccati(in0);
        if (ref.sweep != Sweep::SiDpp) { CHECK(!ref.si_wg[0]); CHECK(!ref.si_wg[1]); }
        if (in0.sweep != SweepPin::Auto) continue;
        for (SweepPin pin : {SweepPin::SiWave, SweepPin::SiWg}) {
            PlanIn in = in0;
            in.sweep = pin;
            const RiccatiPlan p = plan_riccati(in);
            CHECK(same_but_form(p, ref));
            if (ref.sweep != Sweep::SiDpp) { CHECK(!p.si_wg[0]); CHECK(!p.si_wg[1]); }
            else {
                const int b0 = ref.split ? split_first_half(in.B) : in.B;
                CHECK(p.si_wg[0] == (pin == SweepPin::SiWg && ref.si_lanes[0] == 16));
                CHECK(p.si_wg[1] == (pin == SweepPin::SiWg && ref.si_lanes[1] == 16));
                CHECK(ref.si_wg[0] == (ref.si_lanes[0] == 16 && b0 >= SI_WG_MIN_BATCH));
            }
        }
        for (SweepPin pin : {SweepPin::Mfma, SweepPin::Rows}) {   // on an SiDpp plan these pins still select nothing
            if (ref.sweep != Sweep::SiDpp) continue;
            PlanIn in = in0;
            in.sweep = pin;
            const RiccatiPlan p = plan_riccati(in);
            CHECK(same_but_form(p, ref)); CHECK(p.si_wg[0] == ref.si_wg[0]);
        }
    }
    {   // the sweeps the old pins choose between: unchanged, and the new pins leave AUTO's choice
        where = "C4 pins";
        PlanIn in = c4(4096);
        CHECK(plan_riccati(in).sweep == Sweep::Rows);
        in.sweep = SweepPin::Mfma;
        CHECK(plan_riccati(in).sweep == Sweep::Mfma); CHECK(plan_riccati(in).split);
        in.sweep = SweepPin::SiWg;
        CHECK(plan_riccati(in).sweep == Sweep::Rows); CHECK(!plan_riccati(in).si_wg[0]);
        in = c4(256);
        CHECK(plan_riccati(in).sweep == Sweep::Mfma);
        in.sweep = SweepPin::Rows;
        CHECK(plan_riccati(in).sweep == Sweep::Rows);
        in.sweep = SweepPin::SiWave;
        CHECK(plan_riccati(in).sweep == Sweep::Mfma);
    }
    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
