// The sweep pin SweepPin::SiWgPrep and the field RiccatiPlan::si_prep of plan_riccati (ilqr_planner_amd/csrc/ilqr_plan.hpp): the I/O-wave form of
// k_backward_si_dpp with two preparing waves.  The field is true only where si_io is (which is true only where si_wg is); pin 7 forces it there and
// acts as pin 6 elsewhere; pins 4, 5 and 6 turn it off; AUTO adds it from SI_PREP_MIN_BATCH launched instances wherever it takes the I/O wave, so
// never on the halves of a split solve and never on the 8-lane grouping; no pin changes any other field.  Host-only (g++); built and run by
// tests/test_sweep_prep_pin_cpu.py.  n_simd = 1024 throughout.
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "ilqr_hip.h"
#include "ilqr_plan.hpp"

using namespace ilqr;

static int fails = 0;
static const char* where = "";
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { std::printf("FAIL [%s] line %d: %s\n", where, __LINE__, #cond); fails++; } \
    } while (0)

// the inputs of tests/cpp/sweep_io_pin_main.cpp
static PlanIn base(int kind, int nd, bool al, int B) {
    PlanIn in;
    in.kind = kind; in.nd = nd; in.al = al; in.B = B; in.n_simd = 1024; in.halves = B >= SPLIT_MIN_BATCH;
    in.nb_iter = 10; in.uniform_R = true;
    return in;
}
static PlanIn c3(int B, int m = 2) {
    PlanIn in = base(0, 1, true, B);
    in.m = m; in.con_state_only = true;
    return in;
}
static PlanIn c2(int B) { return base(0, 1, false, B); }
static PlanIn c4(int B) { return base(1, 2, false, B); }
static PlanIn with_control_row(PlanIn in, int m = 2) { in.m = m; in.con_state_only = false; return in; }
template <class F>
static PlanIn mod(PlanIn in, F f) { f(in); return in; }

static std::vector<PlanIn> table_inputs() {
    std::vector<PlanIn> v;
    for (int B : {255, 256, 3072, 3073, 4096, 4097, 4100, 8192, 10000}) { v.push_back(c3(B)); v.push_back(c3(B, 1)); v.push_back(c2(B)); }
    for (int B : {256, 1024, 1025, 2048, 2049, 4096}) v.push_back(c4(B));
    v.push_back(mod(c3(4096), [](PlanIn& i) { i.uniform_R = false; }));
    v.push_back(mod(c3(4096, 1), [](PlanIn& i) { i.uniform_R = false; }));
    v.push_back(mod(c3(256, 1), [](PlanIn& i) { i.forward = FwdPin::Wg; }));
    v.push_back(mod(c3(4096, 1), [](PlanIn& i) { i.forward = FwdPin::Dpp; }));
    for (int B : {256, 4096}) {
        v.push_back(with_control_row(base(1, 1, true, B), 17));
        v.push_back(with_control_row(c3(B)));
        v.push_back(with_control_row(c3(B), 1));
        v.push_back(with_control_row(base(2, 1, true, B)));
        for (int m : {1, 2, 4, 5}) {
            v.push_back(mod(c3(B), [m](PlanIn& i) { i.m = m; }));
            v.push_back(mod(base(2, 1, true, B), [m](PlanIn& i) { i.m = m; i.con_state_only = true; }));
        }
        for (int per_step = 0; per_step < 2; per_step++)
            for (int so = 0; so < 2; so++) v.push_back(mod(c3(B), [=](PlanIn& i) { i.m = 1; i.per_step = per_step; i.con_state_only = so != 0; }));
    }
    for (int kind = 0; kind < 4; kind++) {
        v.push_back(mod(base(kind, kind == 1 ? 2 : 1, true, 4096), [](PlanIn& i) { i.m = 1; i.con_state_only = true; i.generic = true; }));
        v.push_back(mod(base(kind, kind == 1 ? 2 : 1, true, 4096), [](PlanIn& i) { i.m = 1; i.con_state_only = true; i.limits2_set = true; }));
    }
    v.push_back(mod(c3(4096, 1), [](PlanIn& i) { i.alpha_floor = 1e-6; }));
    for (int B : {2048, 4096}) v.push_back(mod(c3(B, 1), [](PlanIn& i) { i.off32 = false; }));
    v.push_back(mod(c3(4096, 1), [](PlanIn& i) { i.nb_iter = 0; }));
    v.push_back(mod(c3(4096, 1), [](PlanIn& i) { i.line_search = false; }));
    for (int B : {4096, 8192, 10000}) v.push_back(mod(c3(B, 1), [](PlanIn& i) { i.split = 2; }));
    return v;
}

// every field but si_wg, si_io and si_prep
static bool same_but_form(const RiccatiPlan& a, const RiccatiPlan& b) {
    return a.n_alpha == b.n_alpha && a.init == b.init && a.init_al_update == b.init_al_update && a.sweep == b.sweep && a.si_lanes[0] == b.si_lanes[0] &&
           a.si_lanes[1] == b.si_lanes[1] && a.forward == b.forward && a.fwd_lds == b.fwd_lds && a.apply == b.apply && a.al_update == b.al_update &&
           a.fused == b.fused && a.kd_sym == b.kd_sym && a.split == b.split && a.needs_ws == b.needs_ws;
}

int main() {
    static_assert((int)SweepPin::SiWave == 4 && (int)SweepPin::SiWg == 5 && (int)SweepPin::SiWgIo == 6 && (int)SweepPin::SiWgPrep == 7, "pin values of include/ilqr_hip.h");
    static_assert(ILQR_XC_SWEEP_SI_WAVE == 4 && ILQR_XC_SWEEP_SI_WG == 5 && ILQR_XC_SWEEP_SI_WG_IO == 6 && ILQR_XC_SWEEP_SI_WG_PREP == 7, "pin values");
    static_assert(SI_PREP_MIN_BATCH >= SI_IO_MIN_BATCH, "AUTO takes the preparing waves only where it takes the I/O wave");
    {   // the single-integrator sweep: PosOrn-1 and JointSpace-1, without AL and with 1 .. 4 rows, over batch sizes about every threshold
        for (int kind : {0, 2})
            for (int m = 0; m <= 4; m++)
                for (int B : {1, 5, 16, 17, 67, SI_IO_MIN_BATCH - 1, SI_IO_MIN_BATCH, SI_PREP_MIN_BATCH - 1, SI_PREP_MIN_BATCH, SI_PREP_MIN_BATCH + 1, 1024, 2048,
                              3072, 4096, 4097, 8192}) {
                    if (B < 1) continue;
                    PlanIn in = base(kind, 1, m > 0, B);
                    if (m) { in.m = m; in.con_state_only = true; }
                    const bool lanes16 = B <= 4096, few_rows = m <= 1;
                    where = "AUTO";
                    const RiccatiPlan autop = plan_riccati(in);
                    CHECK(autop.sweep == Sweep::SiDpp); CHECK(autop.si_lanes[0] == (lanes16 ? 16 : 8));
                    CHECK(autop.si_io[0] == (lanes16 && few_rows && B >= SI_IO_MIN_BATCH));
                    CHECK(autop.si_prep[0] == (lanes16 && few_rows && B >= SI_IO_MIN_BATCH && B >= SI_PREP_MIN_BATCH)); CHECK(!autop.si_prep[1]);
                    where = "pin 7 (siwgprep)";
                    in.sweep = SweepPin::SiWgPrep;
                    const RiccatiPlan pr = plan_riccati(in);
                    CHECK(pr.si_prep[0] == (lanes16 && few_rows));  // exactly where 16 lanes and m <= 1 meet
                    CHECK(pr.si_io[0] == pr.si_prep[0]);            // elsewhere what pin 6 gives ...
                    CHECK(pr.si_wg[0] == lanes16);
                    where = "pin 6 (siwgio)";
                    in.sweep = SweepPin::SiWgIo;
                    const RiccatiPlan io = plan_riccati(in);
                    CHECK(!io.si_prep[0]); CHECK(!io.si_prep[1]);
                    CHECK(io.si_io[0] == pr.si_io[0]); CHECK(io.si_io[1] == pr.si_io[1]); CHECK(io.si_wg[0] == pr.si_wg[0]); CHECK(io.si_wg[1] == pr.si_wg[1]);  // ... exactly
                    where = "pin 5 (siwg)";
                    in.sweep = SweepPin::SiWg;
                    const RiccatiPlan wg = plan_riccati(in);
                    CHECK(!wg.si_prep[0]); CHECK(!wg.si_prep[1]); CHECK(!wg.si_io[0]); CHECK(wg.si_wg[0] == pr.si_wg[0]);
                    where = "pin 4 (siwave)";
                    in.sweep = SweepPin::SiWave;
                    const RiccatiPlan wave = plan_riccati(in);
                    CHECK(!wave.si_prep[0]); CHECK(!wave.si_prep[1]); CHECK(!wave.si_io[0]); CHECK(!wave.si_wg[0]);
                    where = "rest of the plan";
                    CHECK(same_but_form(pr, autop)); CHECK(same_but_form(io, autop)); CHECK(same_but_form(wg, autop)); CHECK(same_but_form(wave, autop));
                    where = "pins mfma / rows";  // they select nothing on this sweep
                    for (SweepPin pin : {SweepPin::Mfma, SweepPin::Rows}) {
                        in.sweep = pin;
                        const RiccatiPlan q = plan_riccati(in);
                        CHECK(same_but_form(q, autop)); CHECK(q.si_prep[0] == autop.si_prep[0]); CHECK(q.si_io[0] == autop.si_io[0]); CHECK(q.si_wg[0] == autop.si_wg[0]);
                    }
                }
    }
    {   // split halves: AUTO never gives them the form (it does not give them the I/O wave); the pin follows the launched half
        where = "split 2";
        PlanIn in = c3(8192, 1);
        in.split = 2;
        RiccatiPlan p = plan_riccati(in);  // two halves of 4096
        CHECK(p.split); CHECK(p.si_wg[0]); CHECK(p.si_wg[1]); CHECK(!p.si_io[0]); CHECK(!p.si_io[1]); CHECK(!p.si_prep[0]); CHECK(!p.si_prep[1]);
        in.sweep = SweepPin::SiWgPrep;
        p = plan_riccati(in);
        CHECK(p.si_prep[0]); CHECK(p.si_prep[1]); CHECK(p.si_io[0]); CHECK(p.si_io[1]); CHECK(p.si_wg[0]); CHECK(p.si_wg[1]);
        in.sweep = SweepPin::SiWgIo;
        p = plan_riccati(in);
        CHECK(!p.si_prep[0]); CHECK(!p.si_prep[1]); CHECK(p.si_io[0]); CHECK(p.si_io[1]);
        in = c3(10000, 1);                 // 8 lanes per instance in both halves: never, whatever the pin says
        in.split = 2; in.sweep = SweepPin::SiWgPrep;
        p = plan_riccati(in);
        CHECK(p.si_lanes[0] == 8); CHECK(!p.si_prep[0]); CHECK(!p.si_prep[1]); CHECK(!p.si_io[0]); CHECK(!p.si_io[1]); CHECK(!p.si_wg[0]); CHECK(!p.si_wg[1]);
        in = c3(8192, 1);                  // unsplit, 8 lanes
        for (SweepPin pin : {SweepPin::Auto, SweepPin::SiWgPrep}) {
            in.sweep = pin;
            p = plan_riccati(in);
            CHECK(p.si_lanes[0] == 8); CHECK(!p.si_prep[0]); CHECK(!p.si_io[0]); CHECK(!p.si_wg[0]);
        }
    }
    // every input of the plan table: si_prep => si_io => si_wg, never on another sweep, AUTO by the two thresholds, and none of the four pins changes
    // anything but the three form fields
    for (const PlanIn& in0 : table_inputs()) {
        where = "plan table";
        const RiccatiPlan ref = plan_riccati(in0);
        const bool few_rows = !in0.al || in0.m <= 1;
        const int launched[2] = {ref.split ? split_first_half(in0.B) : in0.B, ref.split ? in0.B - split_first_half(in0.B) : 0};
        for (int h = 0; h < 2; h++) {
            CHECK(!ref.si_prep[h] || ref.si_io[h]);
            CHECK(!ref.si_io[h] || ref.si_wg[h]);
            CHECK(!ref.si_prep[h] || (ref.sweep == Sweep::SiDpp && ref.si_lanes[h] == 16 && few_rows));
            CHECK(ref.si_prep[h] == (ref.si_io[h] && launched[h] >= SI_PREP_MIN_BATCH));
            CHECK(!ref.si_prep[h] || !ref.split);
        }
        for (SweepPin pin : {SweepPin::SiWave, SweepPin::SiWg, SweepPin::SiWgIo, SweepPin::SiWgPrep}) {
            PlanIn in = in0;
            in.sweep = pin;
            const RiccatiPlan p = plan_riccati(in);
            CHECK(same_but_form(p, ref));
            for (int h = 0; h < 2; h++) {
                const bool sidpp16 = ref.sweep == Sweep::SiDpp && ref.si_lanes[h] == 16;
                CHECK(p.si_prep[h] == (pin == SweepPin::SiWgPrep && sidpp16 && few_rows));
                CHECK(p.si_io[h] == ((pin == SweepPin::SiWgIo || pin == SweepPin::SiWgPrep) && sidpp16 && few_rows));
                CHECK(p.si_wg[h] == (pin != SweepPin::SiWave && sidpp16));
            }
        }
    }
    {   // the sweeps the old pins choose between: the new pin leaves AUTO's choice
        where = "C4 pins";
        PlanIn in = c4(4096);
        in.sweep = SweepPin::SiWgPrep;
        CHECK(plan_riccati(in).sweep == Sweep::Rows); CHECK(!plan_riccati(in).si_prep[0]); CHECK(!plan_riccati(in).si_io[0]); CHECK(!plan_riccati(in).si_wg[0]);
        in = c4(256);
        in.sweep = SweepPin::SiWgPrep;
        CHECK(plan_riccati(in).sweep == Sweep::Mfma); CHECK(!plan_riccati(in).si_prep[0]);
    }
    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
