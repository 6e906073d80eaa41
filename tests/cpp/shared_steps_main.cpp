// Keypoints that share a timestep, general mixtures: one SequentialSystem solved on the device (plain KDLRobot: lowered) and over its virtuals
// (SameRobot, a subclass that changes nothing: System::builtin() is false, so csrc/host/ilqr_host_loop.cpp runs the reference's algorithm,
// whose SequentialSystem::cost / cost_x / cost_xx sum the sub-systems' terms as SequentialSystem.cpp:115-160 does).  The sequence holds
//   sub-system A: PosOrnPlannerSys on a TransformedSimulationInterface (object frame): a PosOrnKeypointDistFunct (dead zone) on the final step
//                 and a plain via keypoint at T/2,
//   sub-system B: PosOrnPlannerSys in the base frame: another target on the final step,
//   sub-system C: JointSpacePlannerSys (hybrid sequence): a joint target on the final step and another at T/2,
// so the final step carries three keypoints of three kinds, frames and targets, and step T/2 two.  A plain PosOrnPlannerSys given two
// keypoints on its final step keeps the last one given on both sides (System.cpp:78-80).  ILQRRecursive and AL_ILQR: the same step sizes,
// per-iteration cost within 1e-5 relative (the callback prints six digits), U within 1e-6.  The batch solvers refuse the sequence.
// argv[1] = URDF path; argv[2] = "generic" pins the device library to its lane-per-instance kernels (the host build of tests/tools/hostsim has
// no other).  Exit code 0 = all checks passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../ilqr_planner_amd/csrc/host/ilqr_host.hpp"

using namespace ilqr_planner;

struct SameRobot : sim::KDLRobot {  // changes nothing: still taken over its virtuals (the type decides), so host and device can be compared
    using sim::KDLRobot::KDLRobot;
    void updateKinematics() override { sim::KDLRobot::updateKinematics(); }
};

struct Costs : CallBackMessage {  // "Iteration i, Cost: c, alpha= a"
    std::vector<double> cost, alpha;
    void notify(const std::string& m) override {
        const size_t a = m.find("Cost: "), b = m.find(", alpha= ");
        if (a == std::string::npos || b == std::string::npos) return;
        cost.push_back(std::stod(m.substr(a + 6, b - a - 6)));
        alpha.push_back(std::stod(m.substr(b + 9)));
    }
};

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) { std::printf("FAILED: %s (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

static const int T = 30, DOF = 7;
static const double DT = 0.1;
static const Vec Q0{0.62991112, -0.2329776, -0.01423721, -1.70254115, 0.06251303, 1.50592777, 0.71771416}, DQ0(DOF, 0.0);
static const Vec QMAX{2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973}, QMIN{-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973};

using MakeRobot = std::function<std::shared_ptr<sim::KDLRobot>()>;

static Mat diag(const Vec& v) {
    Mat m((int)v.size(), (int)v.size());
    for (size_t i = 0; i < v.size(); i++) m((int)i, (int)i) = v[i];
    return m;
}

static std::shared_ptr<sys::System> mixture(const MakeRobot& make) {
    auto rbt = make();
    Mat fr = Mat::Identity(4);  // object frame: 0.3 rad about z, then an offset
    const double c = std::cos(0.3), s = std::sin(0.3);
    fr(0, 0) = c; fr(0, 1) = -s; fr(1, 0) = s; fr(1, 1) = c;
    fr(0, 3) = 0.10; fr(1, 3) = -0.05; fr(2, 3) = 0.02;
    auto tr = std::make_shared<sim::TransformedSimulationInterface>(rbt, fr);
    const Vec qt{0.0, 1.0, 0.0, 0.0};
    std::vector<std::shared_ptr<sys::Keypoint>> ka{
        std::make_shared<sys::PosOrnKeypointDistFunct>(Vec{0.30, 0.25, 0.40}, qt, diag({1, 1, 1, .1, .1, .1}), 0.02, Vec{0.05, 0.02, 0.0}, T - 1),
        std::make_shared<sys::PosOrnKeypoint>(Vec{0.35, 0.05, 0.55}, qt, diag({1, 1, 1, 0, 0, 0}), T / 2)};
    std::vector<std::shared_ptr<sys::Keypoint>> kb{std::make_shared<sys::PosOrnKeypoint>(Vec{0.45, 0.10, 0.45}, qt, diag({.5, .5, .5, .05, .05, .05}), T - 1)};
    Vec qc = Q0, qc2 = Q0;
    for (int i = 0; i < DOF; i++) { qc[i] += 0.2 * std::sin(1.0 + i); qc2[i] -= 0.15 * std::cos(2.0 + i); }
    std::vector<std::shared_ptr<sys::Keypoint>> kc{std::make_shared<sys::AngularKeypoint>(qc, diag(Vec(DOF, 0.1)), T - 1),
                                                   std::make_shared<sys::AngularKeypoint>(qc2, diag(Vec(DOF, 0.05)), T / 2)};
    auto A = std::make_shared<sys::PosOrnPlannerSys>(tr, ka, Vec(DOF, 1e-4), QMAX, QMIN, T, 1, DT);
    auto B = std::make_shared<sys::PosOrnPlannerSys>(rbt, kb, Vec(DOF, 1e-5), QMAX, QMIN, T, 1, DT);
    auto C = std::make_shared<sys::JointSpacePlannerSys>(rbt, kc, Vec(DOF, 1e-3), QMAX, QMIN, T, 1, DT);
    return std::make_shared<sys::SequentialSystem>(rbt, std::vector<std::shared_ptr<sys::System>>{A, B, C}, Vec(DOF, 1e-6), T, 1);
}

static std::shared_ptr<sys::System> plain_duplicate(const MakeRobot& make) {  // two keypoints on the final step of a plain System: the last one given counts
    const Vec qt{0.0, 1.0, 0.0, 0.0};
    std::vector<std::shared_ptr<sys::Keypoint>> k{
        std::make_shared<sys::PosOrnKeypoint>(Vec{0.30, 0.25, 0.40}, qt, diag({1, 1, 1, 0, 0, 0}), T - 1),
        std::make_shared<sys::PosOrnKeypoint>(Vec{0.35, 0.05, 0.55}, qt, diag({1, 1, 1, 0, 0, 0}), T / 2),
        std::make_shared<sys::PosOrnKeypoint>(Vec{0.45, 0.10, 0.45}, qt, diag({2, 2, 2, .1, .1, .1}), T - 1)};
    return std::make_shared<sys::PosOrnPlannerSys>(make(), k, Vec(DOF, 1e-5), QMAX, QMIN, T, 1, DT);
}

static int compare(const char* what, const Costs& cd, const Costs& ch, const std::vector<Vec>& Ud, const std::vector<Vec>& Uh, int n) {
    CHECK((int)cd.cost.size() == n && (int)ch.cost.size() == n);
    for (int i = 0; i < n; i++) {
        CHECK(cd.alpha[i] == ch.alpha[i]);
        CHECK(std::fabs(cd.cost[i] - ch.cost[i]) <= 1e-5 * std::fabs(cd.cost[i]) + 1e-12);
    }
    CHECK(Ud.size() == Uh.size());
    double worst = 0;
    for (size_t k = 0; k < Ud.size(); k++)
        for (size_t i = 0; i < Ud[k].size(); i++) worst = std::fmax(worst, std::fabs(Ud[k][i] - Uh[k][i]));
    CHECK(worst <= 1e-6);
    double un = 0;
    for (const Vec& u : Ud)
        for (double v : u) un = std::fmax(un, std::fabs(v));
    std::printf("%s: device and host loop agree (cost %.6g -> %.6g, alpha %g .. %g, max |U| %.3g, max |dU| %.2e)\n", what, cd.cost.front(), cd.cost.back(),
                cd.alpha.front(), cd.alpha.back(), un, worst);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (argc > 2 && std::strcmp(argv[2], "generic") == 0) CHECK(ilqr_ctx_set_crosscheck(device_context(), 1, 0, 0, 0, 0, 0) == 0);
    const std::string urdf = argv[1];
    const MakeRobot dev = [&] { return std::make_shared<sim::KDLRobot>(urdf, "panda_link0", "panda_tip", Q0, DQ0); };
    const MakeRobot host = [&] { return std::make_shared<SameRobot>(urdf, "panda_link0", "panda_tip", Q0, DQ0); };
    const std::vector<Vec> U0(T - 1, Vec(DOF, 0.0));
    const int NIT = 6;

    auto sd = mixture(dev), sh = mixture(host);
    CHECK(sd->builtin() && !sh->builtin());
    {
        Costs cd, ch;
        auto a = solver::ILQRRecursive(sd).solve(U0, NIT, true, false, &cd);
        auto b = solver::ILQRRecursive(sh).solve(U0, NIT, true, false, &ch);
        if (compare("ILQRRecursive, mixture", cd, ch, std::get<2>(a), std::get<2>(b), NIT)) return 1;
    }
    {
        Mat A(1, 2 * DOF);
        A(0, 5) = 1.0;  // q_6 <= 2.0 at every step
        const Vec b{2.0};
        const std::vector<solver::Constraint> con(T - 1, solver::Constraint{A, b});
        const std::vector<Vec> lam(T - 1, b);
        Costs cd, ch;
        auto x = solver::AL_ILQR(sd, con, lam).solve(U0, NIT, 3, 0.25, 1.1, true, false, &cd);
        auto y = solver::AL_ILQR(sh, con, lam).solve(U0, NIT, 3, 0.25, 1.1, true, false, &ch);
        if (compare("AL_ILQR, mixture", cd, ch, std::get<2>(x), std::get<2>(y), NIT)) return 1;
    }
    {
        bool refused = false;
        try {
            Costs cb;
            Mat P((T - 1) * DOF, DOF);
            for (int k = 0; k < T - 1; k++)
                for (int i = 0; i < DOF; i++) P(k * DOF + i, i) = 1.0;
            solver::BatchILQRCP(sd, P).solve(1, Vec((T - 1) * DOF, 0.0), false, &cb);
        } catch (const std::runtime_error& e) {
            refused = std::string(e.what()).find("keypoints that share a timestep are not supported by the batch solvers") != std::string::npos;
        }
        CHECK(refused);
    }
    {
        auto pd = plain_duplicate(dev), ph = plain_duplicate(host);
        CHECK(pd->builtin() && !ph->builtin());
        Costs cd, ch;
        auto a = solver::ILQRRecursive(pd).solve(U0, NIT, true, false, &cd);
        auto b = solver::ILQRRecursive(ph).solve(U0, NIT, true, false, &ch);
        if (compare("ILQRRecursive, plain System with a duplicated step", cd, ch, std::get<2>(a), std::get<2>(b), NIT)) return 1;
    }
    std::printf("ok\n");
    return 0;
}
