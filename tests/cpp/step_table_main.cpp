// Table test of the keypoint step table (ilqr_planner_amd/csrc/ilqr_steps.hpp) and of the plan rows for problems whose keypoints share a
// timestep (ilqr_planner_amd/csrc/ilqr_plan.hpp: PlanIn::shared_steps).  Host-only (g++); built and run by tests/test_shared_steps_cpu.py.
#include <cstdio>
#include <initializer_list>

#include "ilqr_plan.hpp"
#include "ilqr_steps.hpp"

using namespace ilqr;

static int fails = 0;
static const char* where = "";
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { std::printf("FAIL [%s] line %d: %s\n", where, __LINE__, #cond); fails++; } \
    } while (0)

// the table lists the steps of kp_t, expects[s] keypoints on step s
static void check_table(const char* name, const int* kp_t, int n_kp, int n_steps, const int* t, const int* first) {
    where = name;
    StepTable st;
    CHECK(build_step_table(kp_t, n_kp, st));
    CHECK(st.n == n_steps);
    for (int s = 0; s < n_steps && s < STEP_MAX_KP; s++) {
        CHECK(st.t[s] == t[s]);
        CHECK(st.kp[s] == first[s]);
        CHECK(st.kp[s + 1] > st.kp[s]);
        for (int k = st.kp[s]; k < st.kp[s + 1]; k++) CHECK(kp_t[k] == st.t[s]);
    }
    for (int s = n_steps; s <= STEP_MAX_KP; s++) CHECK(st.kp[s] == n_kp);
    CHECK(has_shared_step(st) == (n_steps < n_kp));
}

static PlanIn base(int kind, int nd, bool al, int B) {
    PlanIn in;
    in.kind = kind; in.nd = nd; in.al = al; in.B = B; in.n_simd = 1024; in.halves = B >= SPLIT_MIN_BATCH;
    in.nb_iter = 10; in.uniform_R = true;
    return in;
}

static void check_generic(const RiccatiPlan& p) {
    CHECK(p.init == Init::Generic); CHECK(!p.init_al_update);
    CHECK(p.sweep == Sweep::Generic); CHECK(p.forward == Forward::Generic); CHECK(p.apply == Apply::None);
    CHECK(!p.al_update); CHECK(!p.fused); CHECK(p.kd_sym == 0); CHECK(!p.split); CHECK(p.needs_ws);
}

int main() {
    {   // unique timesteps: step s is keypoint s
        const int kp_t[] = {3, 7, 19}, t[] = {3, 7, 19}, first[] = {0, 1, 2};
        check_table("unique", kp_t, 3, 3, t, first);
    }
    {
        const int t[] = {0}, first[] = {0};
        check_table("empty", nullptr, 0, 0, t, first);
    }
    {   // runs of shared steps between unique ones
        const int kp_t[] = {0, 4, 4, 4, 9, 12, 12, 19}, t[] = {0, 4, 9, 12, 19}, first[] = {0, 1, 4, 5, 7};
        check_table("runs", kp_t, 8, 5, t, first);
    }
    {   // all keypoints on one step
        const int kp_t[] = {5, 5, 5, 5, 5, 5, 5, 5}, t[] = {5}, first[] = {0};
        check_table("all on one step", kp_t, 8, 1, t, first);
    }
    {   // two keypoints on the final step of a T = 20 horizon
        const int kp_t[] = {10, 19, 19}, t[] = {10, 19}, first[] = {0, 1};
        check_table("final step", kp_t, 3, 2, t, first);
    }
    {   // one keypoint, at step 0
        const int kp_t[] = {0}, t[] = {0}, first[] = {0};
        check_table("single", kp_t, 1, 1, t, first);
    }
    {
        where = "rejected";
        StepTable st;
        const int dec[] = {4, 3};
        CHECK(!build_step_table(dec, 2, st)); CHECK(st.n == 0);
        const int nine[] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
        CHECK(!build_step_table(nine, 9, st));
        CHECK(!build_step_table(nine, -1, st));
    }

    // shared steps run on the generic kernels for every shape, batch size and pin; without them the plan is the plan of the cooperative set
    for (int kind = 0; kind < 4; kind++) {
        for (int nd = 1; nd <= 2; nd++) {
            if (kind >= 2 && nd == 2) continue;
            for (int al = 0; al < 2; al++) {
                for (int B : {13, 256, 2048, 2049, 3072, 3073, 4096, 4100}) {
                    for (int pin = 0; pin < 3; pin++) {
                        where = "shared steps";
                        PlanIn in = base(kind, nd, al != 0, B);
                        if (al) { in.m = 2; in.con_state_only = true; }
                        in.sweep = (SweepPin)pin; in.forward = (FwdPin)pin; in.reroll = (RerollPin)pin;
                        PlanIn sh = in;
                        sh.shared_steps = true;
                        check_generic(plan_riccati(sh));
                        sh.split = 2;
                        check_generic(plan_riccati(sh));
                        where = "unique steps";
                        PlanIn gen = in;
                        gen.generic = true;
                        const RiccatiPlan a = plan_riccati(sh), b = plan_riccati(gen);
                        CHECK(a.sweep == b.sweep && a.forward == b.forward && a.apply == b.apply && a.init == b.init);
                        CHECK(plan_riccati(in).sweep != Sweep::Generic);
                    }
                }
            }
        }
    }
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
