// The decision table of plan_riccati (ilqr_planner_amd/csrc/ilqr_plan.hpp): which kernels a Riccati solve runs for a given shape, batch size
// and pin set.  Host-only (g++); built and run by tests/test_plan_cpu.py.  n_simd = 1024 (MI355X: 256 CUs) throughout.
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

static PlanIn base(int kind, int nd, bool al, int B) {
    PlanIn in;
    in.kind = kind; in.nd = nd; in.al = al; in.B = B; in.n_simd = 1024; in.halves = B >= SPLIT_MIN_BATCH;
    in.nb_iter = 10; in.uniform_R = true;
    return in;
}
// C3: PosOrn-1 AL, two shared state-only rows, uniform control weights
static PlanIn c3(int B) {
    PlanIn in = base(0, 1, true, B);
    in.m = 2; in.con_state_only = true;
    return in;
}
static PlanIn c2(int B) { return base(0, 1, false, B); }  // PosOrn-1 recursive
static PlanIn c4(int B) { return base(1, 2, false, B); }  // PosOrnTime-2 recursive
static PlanIn with_control_row(PlanIn in, int m = 2) { in.m = m; in.con_state_only = false; return in; }

int main() {
    {
        where = "C3 4096";
        const RiccatiPlan p = plan_riccati(c3(4096));
        CHECK(p.n_alpha == 11);
        CHECK(p.init == Init::Lti); CHECK(!p.init_al_update);
        CHECK(p.sweep == Sweep::SiDpp); CHECK(p.si_lanes[0] == 16);
        CHECK(p.forward == Forward::WaveWg);
        CHECK(p.apply == Apply::WaveLast); CHECK(p.fused); CHECK(!p.al_update);
        CHECK(p.kd_sym == 1); CHECK(!p.split); CHECK(!p.needs_ws);
    }
    where = "C3 forward threshold";
    CHECK(plan_riccati(c3(3072)).forward == Forward::WaveDpp);
    CHECK(plan_riccati(c3(3073)).forward == Forward::WaveWg);
    where = "C3 si lanes threshold";
    CHECK(plan_riccati(c3(4096)).si_lanes[0] == 16);
    CHECK(plan_riccati(c3(4097)).si_lanes[0] == 8);
    CHECK(plan_riccati(c3(4100)).si_lanes[0] == 8);
    CHECK(plan_riccati(c3(4100)).sweep == Sweep::SiDpp);
    {
        where = "C3, R not uniform";
        PlanIn in = c3(4096);
        in.uniform_R = false;
        const RiccatiPlan p = plan_riccati(in);
        CHECK(p.kd_sym == 0); CHECK(p.fused); CHECK(p.apply == Apply::WaveLast);
    }
    {
        where = "C2 256";
        const RiccatiPlan p = plan_riccati(c2(256));
        CHECK(p.sweep == Sweep::SiDpp); CHECK(p.si_lanes[0] == 16);
        CHECK(p.forward == Forward::WaveDpp); CHECK(p.fused); CHECK(p.apply == Apply::WaveLast);
        CHECK(p.init == Init::Lti); CHECK(!p.init_al_update); CHECK(!p.al_update);
    }
    {
        where = "C4 4096";
        const RiccatiPlan p = plan_riccati(c4(4096));
        CHECK(p.init == Init::Lti); CHECK(!p.init_al_update);
        CHECK(p.sweep == Sweep::Rows); CHECK(p.forward == Forward::Mfma); CHECK(p.apply == Apply::RerollRows);
        CHECK(!p.al_update); CHECK(!p.fused); CHECK(p.kd_sym == 0); CHECK(!p.split); CHECK(!p.needs_ws);
    }
    {
        where = "C4 2048";
        const RiccatiPlan p = plan_riccati(c4(2048));
        CHECK(p.sweep == Sweep::Mfma); CHECK(p.split); CHECK(p.apply == Apply::RerollRows);
        CHECK(split_first_half(2048) == 1024);
    }
    where = "C4 rows sweep threshold";
    CHECK(plan_riccati(c4(2048)).sweep == Sweep::Mfma);
    CHECK(plan_riccati(c4(2049)).sweep == Sweep::Rows);
    CHECK(!plan_riccati(c4(2049)).split);
    where = "C4 re-roll threshold";
    CHECK(plan_riccati(c4(1024)).apply == Apply::RerollDpp);
    CHECK(plan_riccati(c4(1025)).apply == Apply::RerollRows);
    CHECK(!plan_riccati(c4(1024)).split);  // no halves below SPLIT_MIN_BATCH
    {
        where = "C4, line search off";
        PlanIn in = c4(4096);
        in.line_search = false;
        const RiccatiPlan p = plan_riccati(in);
        CHECK(p.n_alpha == 1); CHECK(p.forward == Forward::Mfma); CHECK(p.apply == Apply::None);
    }
    {
        where = "C4 pins";
        PlanIn in = c4(4096);
        in.sweep = SweepPin::Mfma;
        CHECK(plan_riccati(in).sweep == Sweep::Mfma); CHECK(plan_riccati(in).split);
        in = c4(256);
        in.sweep = SweepPin::Rows; in.reroll = RerollPin::Rows;
        CHECK(plan_riccati(in).sweep == Sweep::Rows); CHECK(plan_riccati(in).apply == Apply::RerollRows);
        in = c4(4096);
        in.reroll = RerollPin::Dpp;
        CHECK(plan_riccati(in).apply == Apply::RerollDpp);
        in = c3(256);
        in.forward = FwdPin::Wg;
        CHECK(plan_riccati(in).forward == Forward::WaveWg);
        in = c3(4096);
        in.forward = FwdPin::Dpp;
        CHECK(plan_riccati(in).forward == Forward::WaveDpp);
    }
    for (int B : {256, 4096}) {
        where = "PosOrnTime AL, m 17";
        PlanIn in = with_control_row(base(1, 1, true, B), 17);
        const RiccatiPlan p = plan_riccati(in);
        CHECK(p.sweep == Sweep::Generic); CHECK(p.needs_ws);
        CHECK(p.forward == Forward::Mfma); CHECK(p.apply == (B == 256 ? Apply::RerollDpp : Apply::RerollRows));
        CHECK(p.al_update); CHECK(p.init == Init::Lti); CHECK(p.init_al_update); CHECK(!p.split);
    }
    for (int B : {256, 4096}) {
        where = "PosOrn-2 AL, m 16";
        PlanIn in = with_control_row(base(0, 2, true, B), 16);
        const RiccatiPlan p = plan_riccati(in);
        CHECK(p.sweep == (B == 256 ? Sweep::Mfma : Sweep::Rows));
        CHECK(p.forward == Forward::Lin); CHECK(p.apply == Apply::Lin); CHECK(p.al_update);
        CHECK(p.init == Init::Lti); CHECK(p.init_al_update); CHECK(!p.fused); CHECK(p.kd_sym == 0);
    }
    {
        where = "PosOrn-1 AL with a control row, 4096";
        const RiccatiPlan p = plan_riccati(with_control_row(c3(4096)));
        CHECK(p.sweep == Sweep::Mfma); CHECK(p.split);
        CHECK(p.forward == Forward::WaveWg); CHECK(!p.fused); CHECK(p.apply == Apply::Wave); CHECK(!p.al_update);
        CHECK(p.kd_sym == 0); CHECK(p.init_al_update); CHECK(!p.needs_ws);
    }
    {
        where = "JointSpace-1 AL with a control row, 256";
        PlanIn in = with_control_row(base(2, 1, true, 256));
        const RiccatiPlan p = plan_riccati(in);
        CHECK(p.sweep == Sweep::Generic); CHECK(p.needs_ws);
        CHECK(p.forward == Forward::WaveDpp); CHECK(!p.fused); CHECK(p.apply == Apply::Wave);
        CHECK(p.init == Init::Lti); CHECK(p.init_al_update); CHECK(p.kd_sym == 0);
    }
    for (int B : {256, 4096}) {
        // the register-resident sweep holds at most 4 shared state-only rows: one more row, one set per step or a control row leave it --
        // PosOrn-1 for the matrix-core sweep (k_apply does the AL bookkeeping), JointSpace-1 for the generic sweep and its workspace
        where = "PosOrn-1 AL, m 4 / 5";
        PlanIn in = c3(B);
        in.m = 4;
        RiccatiPlan p = plan_riccati(in);
        CHECK(p.sweep == Sweep::SiDpp); CHECK(p.fused); CHECK(p.apply == Apply::WaveLast); CHECK(p.kd_sym == 1);
        CHECK(!p.al_update); CHECK(!p.init_al_update); CHECK(!p.needs_ws); CHECK(!p.split);
        in.m = 5;
        p = plan_riccati(in);
        CHECK(p.sweep == Sweep::Mfma); CHECK(!p.fused); CHECK(p.apply == Apply::Wave); CHECK(p.kd_sym == 0);
        CHECK(!p.al_update); CHECK(p.init_al_update); CHECK(!p.needs_ws); CHECK(p.split == (B == 4096));
        for (int per_step = 0; per_step < 2; per_step++) {
            for (int state_only = 0; state_only < 2; state_only++) {
                where = "PosOrn-1 AL, m 4, per_step x con_state_only";
                in = c3(B);
                in.m = 4; in.per_step = per_step; in.con_state_only = state_only != 0;
                p = plan_riccati(in);
                const bool si = !per_step && state_only;
                CHECK(p.sweep == (si ? Sweep::SiDpp : Sweep::Mfma)); CHECK(p.fused == si); CHECK(!p.needs_ws);
                CHECK(p.apply == (si ? Apply::WaveLast : Apply::Wave)); CHECK(p.init_al_update == !si);
                where = "JointSpace-1 AL, m 4, per_step x con_state_only";
                in = base(2, 1, true, B);
                in.m = 4; in.per_step = per_step; in.con_state_only = state_only != 0;
                p = plan_riccati(in);
                CHECK(p.sweep == (si ? Sweep::SiDpp : Sweep::Generic)); CHECK(p.fused == si); CHECK(p.needs_ws == !si);
                CHECK(p.forward == (B == 256 ? Forward::WaveDpp : Forward::WaveWg)); CHECK(p.init == Init::Lti);
            }
        }
        where = "JointSpace-1 AL, m 4 / 5";
        in = base(2, 1, true, B);
        in.m = 4; in.con_state_only = true;
        CHECK(plan_riccati(in).sweep == Sweep::SiDpp); CHECK(!plan_riccati(in).needs_ws);
        in.m = 5;
        p = plan_riccati(in);
        CHECK(p.sweep == Sweep::Generic); CHECK(p.needs_ws); CHECK(!p.fused); CHECK(p.apply == Apply::Wave); CHECK(p.init_al_update);
        CHECK(!p.al_update); CHECK(!p.split);
        // 16 rows fit the LDS of the matrix-core sweep and the lanes of an instance's group in the row-per-lane sweep; 17 do not
        for (int nd = 1; nd <= 2; nd++) {
            for (int kind : {0, 1, 3}) {
                if (kind == 3 && nd == 2) continue;
                where = "AL, m 16 / 17";
                in = base(kind, nd, true, B);
                in.m = 16; in.con_state_only = true;
                p = plan_riccati(in);
                const bool rows_ok = !(kind == 0 && nd == 1);
                CHECK(p.sweep == (B == 4096 && rows_ok ? Sweep::Rows : Sweep::Mfma)); CHECK(!p.needs_ws);
                in.sweep = SweepPin::Rows;
                CHECK(plan_riccati(in).sweep == (rows_ok ? Sweep::Rows : Sweep::Mfma));
                in.sweep = SweepPin::Mfma;
                CHECK(plan_riccati(in).sweep == Sweep::Mfma);
                for (SweepPin pin : {SweepPin::Auto, SweepPin::Mfma, SweepPin::Rows}) {
                    in.m = 17; in.sweep = pin;
                    p = plan_riccati(in);
                    CHECK(p.sweep == Sweep::Generic); CHECK(p.needs_ws); CHECK(!p.fused); CHECK(p.kd_sym == 0);
                    CHECK(p.forward != Forward::Generic); CHECK(p.init == Init::Lti); CHECK(p.init_al_update);
                    CHECK(p.al_update == !(kind == 0 && nd == 1));  // (the wave path updates the multipliers in k_apply)
                    CHECK(p.split == false);
                }
            }
        }
    }
    for (int kind = 0; kind < 4; kind++) {
        for (int generic = 0; generic < 2; generic++) {
            where = generic ? "pin generic" : "limits2_set";
            const int nd = kind == 1 ? 2 : 1;
            PlanIn in = base(kind, nd, true, 4096);
            in.m = 2; in.con_state_only = true;
            if (generic) in.generic = true;
            else in.limits2_set = true;
            const RiccatiPlan p = plan_riccati(in);
            CHECK(p.init == Init::Generic); CHECK(!p.init_al_update);
            CHECK(p.sweep == Sweep::Generic); CHECK(p.needs_ws);
            CHECK(p.forward == Forward::Generic); CHECK(p.apply == Apply::None); CHECK(!p.al_update);
            CHECK(!p.fused); CHECK(p.kd_sym == 0); CHECK(!p.split);
        }
    }
    {
        where = "C3, alpha_floor 1e-6";
        PlanIn in = c3(4096);
        in.alpha_floor = 1e-6;
        const RiccatiPlan p = plan_riccati(in);
        CHECK(p.n_alpha == 21);
        CHECK(p.init == Init::Lti); CHECK(p.init_al_update);
        CHECK(p.sweep == Sweep::SiDpp); CHECK(p.forward == Forward::Generic); CHECK(p.apply == Apply::None);
        CHECK(!p.fused); CHECK(p.kd_sym == 0); CHECK(!p.al_update); CHECK(!p.split);
    }
    {
        where = "n_alpha_of at its edges";
        CHECK(n_alpha_of(true, 0.125) == 4);   // the floor is a step size: 1, 1/2, 1/4, 1/8
        CHECK(n_alpha_of(true, 0.1) == 5);     // 1/8 > 0.1 goes on to 1/16
        CHECK(n_alpha_of(true, 1e-3) == 11);
        CHECK(n_alpha_of(true, 4e-5) == 16);   // 2^-15 = 3.05e-5: the last count the cooperative forward passes hold
        CHECK(n_alpha_of(true, 2e-5) == 17);   // the first one past them
        CHECK(n_alpha_of(true, 1e-6) == 21);
        CHECK(n_alpha_of(true, 0.0) == 64);    // capped
        CHECK(n_alpha_of(false, 1e-3) == 1); CHECK(n_alpha_of(false, 1e-6) == 1);  // no line search
    }
    for (int B : {256, 2048, 4096}) {
        // more than 16 step sizes: the cooperative sweeps stay, the forward pass is the generic one, which applies its own winner and (AL) does the
        // multiplier update itself; nothing is split
        for (double floor : {2e-5, 1e-6}) {
            for (int al = 0; al < 2; al++) {
                where = "C2nd, alpha_floor < 2^-15";
                PlanIn in = base(0, 2, al != 0, B);
                if (al) { in.m = 2; in.con_state_only = true; }
                in.alpha_floor = floor;
                RiccatiPlan p = plan_riccati(in);
                CHECK(p.n_alpha == (floor == 2e-5 ? 17 : 21));
                CHECK(p.sweep == (B == 4096 ? Sweep::Rows : Sweep::Mfma)); CHECK(p.forward == Forward::Generic); CHECK(p.apply == Apply::None);
                CHECK(!p.al_update); CHECK(!p.split); CHECK(!p.fused); CHECK(p.kd_sym == 0); CHECK(!p.needs_ws);
                CHECK(p.init == Init::Lti); CHECK(p.init_al_update == (al != 0));
                where = "C4, alpha_floor < 2^-15";
                in = base(1, 2, al != 0, B);
                if (al) { in.m = 2; in.con_state_only = true; }
                in.alpha_floor = floor;
                p = plan_riccati(in);
                CHECK(p.sweep == (B == 4096 ? Sweep::Rows : Sweep::Mfma)); CHECK(p.forward == Forward::Generic); CHECK(p.apply == Apply::None);
                CHECK(!p.al_update); CHECK(!p.split); CHECK(!p.fused); CHECK(p.kd_sym == 0); CHECK(!p.needs_ws);
                in.sweep = SweepPin::Mfma; in.reroll = RerollPin::Dpp;
                p = plan_riccati(in);
                CHECK(p.sweep == Sweep::Mfma); CHECK(p.forward == Forward::Generic); CHECK(p.apply == Apply::None); CHECK(!p.split);
            }
        }
        where = "C4, alpha_floor 4e-5";  // sixteen step sizes are still cooperative
        PlanIn in = c4(B);
        in.alpha_floor = 4e-5;
        const RiccatiPlan p = plan_riccati(in);
        CHECK(p.n_alpha == 16); CHECK(p.forward == Forward::Mfma); CHECK(p.apply != Apply::None);
    }
    for (int B : {2048, 4096}) {
        where = "C3, off32 false";
        PlanIn in = c3(B);
        in.off32 = false;
        const RiccatiPlan p = plan_riccati(in);
        CHECK(p.sweep == Sweep::Mfma); CHECK(p.split); CHECK(!p.fused); CHECK(p.kd_sym == 0); CHECK(p.apply == Apply::Wave);
    }
    for (PlanIn in : {c3(4096), c4(2048), with_control_row(base(2, 1, true, 256))}) {
        where = "nb_iter 0";
        in.nb_iter = 0;
        const RiccatiPlan p = plan_riccati(in);
        CHECK(!p.split); CHECK(!p.needs_ws); CHECK(p.kd_sym == KD_SYM_KEEP);
    }
    {
        where = "profiling on";
        PlanIn in = c4(2048);
        in.profile = true;
        CHECK(!plan_riccati(in).split);
    }
    {
        where = "split 0";
        PlanIn in = c4(2048);
        in.split = 0;
        CHECK(!plan_riccati(in).split);
    }
    {
        where = "split 2";
        PlanIn in = c3(4096);
        in.split = 2;
        RiccatiPlan p = plan_riccati(in);
        CHECK(p.split); CHECK(p.sweep == Sweep::SiDpp); CHECK(p.si_lanes[0] == 16); CHECK(p.si_lanes[1] == 16);
        in = c3(10000);
        in.split = 2;
        p = plan_riccati(in);  // the lane count follows the launched half: 5056 and 4944 instances
        CHECK(p.split); CHECK(p.si_lanes[0] == 8); CHECK(p.si_lanes[1] == 8);
        in = c3(8192);
        in.split = 2;
        p = plan_riccati(in);  // two halves of 4096
        CHECK(p.split); CHECK(p.si_lanes[0] == 16); CHECK(p.si_lanes[1] == 16);
        CHECK(plan_riccati(c3(8192)).si_lanes[0] == 8);  // unsplit
        in = with_control_row(base(2, 1, true, 4096));
        in.split = 2;
        p = plan_riccati(in);
        CHECK(p.split); CHECK(p.sweep == Sweep::Generic); CHECK(p.needs_ws);
    }
    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
