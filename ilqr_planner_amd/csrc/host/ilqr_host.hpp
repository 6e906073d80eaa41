// ilqr_host.hpp -- C++ host mirror of the reference's user-facing classes for the batched iLQR hot path.
//
// Same names, argument meaning and error behaviour (std::runtime_error) as idiap/ilqr_planner:
//   sim::SimulationInterface / sim::KDLRobot          include/ilqr_planner/sim/{SimulationInterface,KDLRobot}.h
//   sys::Keypoint / PosOrnKeypoint / SpacetimeKeypoint include/ilqr_planner/system/*Keypoint.h
//   sys::System / PosOrnPlannerSys / PosOrnTimePlannerSys  include/ilqr_planner/system/{System,PosOrn*PlannerSys}.h
//   solver::ILQRRecursive / AL_ILQR / BatchILQR / BatchILQRCP / LQT  include/ilqr_planner/solver/*.h
//   primitives, Sd, CallBackMessage                   include/ilqr_planner/utils/*.h
// No Eigen (absent from this image): Vec/Mat are plain row-major containers.  These classes hold state and LOWER it to
// the POD descriptor of include/ilqr_hip.h; every solve and every kinematics evaluation runs on the GPU through that C
// ABI -- there is no host solver for them (user-defined System / Keypoint subclasses, which have no descriptor, run
// solver::ILQRRecursive over their own virtuals: ilqr_host_loop.cpp).  The single-point System API (forwardPass, cost*, getFxJac, fpBatch ...) is host glue over
// the simulator for users who call it directly; the solvers never use it.
#pragma once

#include <functional>
#include <memory>
#include <typeinfo>
#include <string>
#include <tuple>
#include <vector>

#include "../../../include/ilqr_hip.h"

namespace ilqr_planner {

using Vec = std::vector<double>;
struct Mat {
    int rows = 0, cols = 0;
    std::vector<double> d;  // row-major
    Mat() {}
    Mat(int r, int c) : rows(r), cols(c), d((size_t)r * c, 0.0) {}
    double& operator()(int r, int c) { return d[(size_t)r * cols + c]; }
    double operator()(int r, int c) const { return d[(size_t)r * cols + c]; }
    static Mat Identity(int n) { Mat m(n, n); for (int i = 0; i < n; i++) m(i, i) = 1; return m; }
};

class CallBackMessage {  // include/ilqr_planner/utils/CallbackMessage.h:12-16
public:
    virtual ~CallBackMessage() {}
    virtual void notify(const std::string& msg) = 0;
};

// process-wide device context (one MI355X per process, as one-rank-per-GPU launches expect)
ilqr_ctx* device_context();
void check(int rc);  // non-zero -> std::runtime_error(ilqr_last_error)

namespace Sd {  // include/ilqr_planner/utils/sd.h
Mat dQuatToDxJac(const Vec& q);
Vec expMap(Vec base, const Vec& u);
double distance(const Vec& x, const Vec& y);
Vec logMap(Vec base, Vec y);
Vec transport(const Vec& v, const Vec& base1, const Vec& base2);
}  // namespace Sd

Mat buildPsiRBF(int dim, int K);  // src/utils/primitives.cpp:19-96
Mat buildPsiBernstein(int dim, int K);
Mat buildPsiUnitstep(int dim, int K);
Mat buildPsiSawtooth(int dim, int K);
Mat buildPsiLinear(int dim, int K);

namespace sim {
class SimulationInterface {  // SimulationInterface.h:13-124
public:
    virtual ~SimulationInterface() {}
    virtual void updateKinematics() = 0;
    Mat Jt();
    Mat Jr();
    virtual Mat J() { return Jac; }
    Mat Jtp();  // rows of Jp(), SimulationInterface.cpp:41-47
    Mat Jrp();
    virtual Mat Jp() { return dJac; }  // dJ/dt (:53-55)
    Mat dQuatToDxJac(const Vec& quat) { return Sd::dQuatToDxJac(quat); }
    virtual void sendAcc(double dt, const Vec& ddq, bool updateKin = true);
    virtual void sendVel(double dt, const Vec& dq, bool updateKin = true);
    virtual Vec getEEPosition() { return x; }
    virtual Vec getEEVelocity() { return dx; }
    virtual Vec getEEAngVel() { return w; }
    Vec getEEAngVelQuat();
    virtual Vec getEEOrnQuat() { return ornQuat; }
    Vec getJointsPos() { return q; }
    Vec getJointsVel() { return dq; }
    int getDOF() { return dof; }
    int getNbCarDim() { return nbCarDim; }
    double getTime() { return t; }
    virtual void setTime(double time) { t = time; }
    virtual void setConfiguration(const Vec& q, const Vec& dq, bool reset_time = true);
    // lowering hook: fill the chain part of the descriptor; false if this simulator cannot run on the device
    virtual bool lowerChain(ilqr_problem_desc*) const { return false; }
    // Is this object EXACTLY one of the simulators of this header (and, for a wrapper, is the wrapped one)?  A user subclass -- also one of
    // sim::KDLRobot that overrides the kinematics or the integrator -- inherits lowerChain() but not this: the device would solve it with
    // the base class's chain and dynamics, so the solvers take such a simulator over its virtuals instead (System::builtin()).
    virtual bool builtinSim() const { return false; }
    // object frame this simulator reports poses in (TransformedSimulationInterface): row-major R[9], p[3]; false = base frame
    virtual bool frame(double*, double*) const { return false; }

protected:
    Vec q, dq, ddq, x, dx, ornQuat, w;
    Mat Jac, dJac;
    int dof = 0, nbCarDim = 3;
    double t = 0;
};

class KDLRobot : public SimulationInterface {  // KDLRobot.h:22-57
public:
    KDLRobot(const std::string& urdf, const std::string& baseFrame, const std::string& tipFrame, const Vec& q, const Vec& dq,
             const Vec& transform_rpy, const Vec& transform_xyz, const bool& is_path);
    KDLRobot(const std::string& urdf, const std::string& baseFrame, const std::string& tipFrame, const Vec& q, const Vec& dq)
        : KDLRobot(urdf, baseFrame, tipFrame, q, dq, Vec(3, 0.0), Vec(3, 0.0), true) {}
    KDLRobot(const std::string& urdf, const std::string& baseFrame, const std::string& tipFrame, const Vec& q, const Vec& dq,
             const Vec& transform_rpy, const Vec& transform_xyz)
        : KDLRobot(urdf, baseFrame, tipFrame, q, dq, transform_rpy, transform_xyz, true) {}
    void updateKinematics() override;  // one-configuration call of ilqr_fk_batch (the FK kernel), then dx = Jt dq, w = Jr dq
    bool lowerChain(ilqr_problem_desc* d) const override;
    bool builtinSim() const override { return typeid(*this) == typeid(KDLRobot); }
    Vec jointLowerLimits() const { return lower_; }
    Vec jointUpperLimits() const { return upper_; }

protected:
    ilqr_problem_desc chain_;  // only the chain fields are meaningful
    Vec lower_, upper_;
};
// Planar arm of 2DRobot.h / 2DRobot.cpp:13-74 (host only: x = sum_i l_i [cos q_i, sin q_i] with ABSOLUTE joint angles, Jacobian by
// forward differences of step pi*1e-3, J = [Jt; 0] (4 x dof), identity quaternion).  Only joint-space systems work with it.
class Robot2D : public SimulationInterface {
public:
    Robot2D(const Vec& lengths, const Vec& default_q);
    Vec fkine(const Vec& q);
    Vec fkine() { return fkine(q); }
    void updateKinematics() override;
    bool builtinSim() const override { return typeid(*this) == typeid(Robot2D); }

protected:
    Vec lengths_;
};

// The wrapped robot seen from an object frame T (4x4 pose): p' = R'(p - t), R_ee' = R' R_ee, J' = blkdiag(R,R)' J
// (TransformedSimulationInterface.h / .cpp:20-103).  The Python constructor takes (robot, T) as the reference's binding does.
class TransformedSimulationInterface : public SimulationInterface {
public:
    TransformedSimulationInterface(const std::shared_ptr<SimulationInterface>& r, const Mat& T);
    void updateKinematics() override;
    Mat J() override;
    Mat Jp() override;
    Vec getEEPosition() override;
    Vec getEEVelocity() override;
    Vec getEEAngVel() override;
    Vec getEEOrnQuat() override;
    void sendAcc(double dt, const Vec& ddq, bool updateKin = true) override;
    void sendVel(double dt, const Vec& dq, bool updateKin = true) override;
    void setConfiguration(const Vec& q, const Vec& dq, bool reset_time = true) override;
    void setTime(double time) override;
    bool lowerChain(ilqr_problem_desc* d) const override { return r_->lowerChain(d); }
    bool builtinSim() const override { return typeid(*this) == typeid(TransformedSimulationInterface) && r_ && r_->builtinSim(); }
    bool frame(double* R, double* p) const override;

protected:
    std::shared_ptr<SimulationInterface> r_;
    Mat T_;
};
}  // namespace sim

namespace sys {
class Keypoint {  // Keypoint.h:15-41
public:
    enum KpType { FIRST_ORDER = 1, SECOND_ORDER = 2 };
    Keypoint(int timestep, KpType type, const std::string& TAG) : TAG_(TAG), type_(type), timestep_(timestep) {}
    virtual ~Keypoint() {}
    virtual Vec diff(const Vec& state) const = 0;
    virtual Vec getState() const = 0;
    virtual Mat getPrecision() const = 0;
    virtual Vec targetFx() const = 0;  // target in f(x) order [p, quat, (dp, dquat), (t)] -- what the device consumes
    int getTimestep() const { return timestep_; }
    std::string getTAG() const { return TAG_; }
    KpType getType() const { return type_; }

protected:
    std::string TAG_;
    KpType type_;
    int timestep_;
};

class PosOrnKeypoint : public Keypoint {  // PosOrnKeypoint.h:15-60
public:
    PosOrnKeypoint(const Vec& position, const Vec& orientation, const Mat& precision, const int& timestep);
    PosOrnKeypoint(const Vec& position, const Vec& dposition, const Vec& orientation, const Vec& dorientation, const Mat& precision, const int& timestep);
    Vec getPosition() const { return position_; }
    Vec getOrientation() const { return orientation_; }
    Mat getPrecision() const override { return precision_; }
    Vec diff(const Vec& state) const override;
    Vec getState() const override;
    Vec targetFx() const override;

protected:
    Vec position_, orientation_, dposition_, dorientation_;
    Mat precision_;
    int state_size_;
};

class PosOrnKeypointDistFunct : public PosOrnKeypoint {  // PosOrnKeypointDistFunct.h:15-44
public:
    PosOrnKeypointDistFunct(const Vec& position, const Vec& orientation, const Mat& precision, const double& pos_radius, const Vec& orn_thresh, const int& timestep);
    PosOrnKeypointDistFunct(const Vec& position, const Vec& dposition, const Vec& orientation, const Vec& dorientation, const Mat& precision,
                            const double& pos_radius, const Vec& orn_thresh, const int& timestep);
    Vec diff(const Vec& state) const override;  // PosOrnKeypointDistFunct.cpp:13-35
    double getPosRadius() const { return pos_radius_; }
    Vec getOrnThresh() const { return orn_thresh_; }

protected:
    double pos_radius_;
    Vec orn_thresh_;
};

class AngularKeypoint : public Keypoint {  // AngularKeypoint.h:15-45: joint-space target, residual = target - state
public:
    AngularKeypoint(const Vec& position, const Mat& precision, const int& timestep)
        : Keypoint(timestep, FIRST_ORDER, "JNT"), position_(position), precision_(precision) {}
    AngularKeypoint(const Vec& position, const Vec& dposition, const Mat& precision, const int& timestep)
        : Keypoint(timestep, SECOND_ORDER, "JNT"), position_(position), dposition_(dposition), precision_(precision) {}
    Vec getPosition() const { return position_; }
    Mat getPrecision() const override { return precision_; }
    Vec diff(const Vec& state) const override;
    Vec getState() const override;
    Vec targetFx() const override { return getState(); }

protected:
    Vec position_, dposition_;
    Mat precision_;
};

class AngularTimeKeypoint : public AngularKeypoint {  // AngularTimeKeypoint.h: joint target + continuous time
public:
    AngularTimeKeypoint(const Vec& position, const Mat& precision, const double& continuous_time, const int& timestep)
        : AngularKeypoint(position, precision, timestep), continuous_time_(continuous_time) { TAG_ = "JNT_TIME"; }
    AngularTimeKeypoint(const Vec& position, const Vec& dposition, const Mat& precision, const double& continuous_time, const int& timestep)
        : AngularKeypoint(position, dposition, precision, timestep), continuous_time_(continuous_time) { TAG_ = "JNT_TIME"; }
    double getContinuousTime() { return continuous_time_; }
    Vec diff(const Vec& state) const override;
    Vec getState() const override;

protected:
    double continuous_time_;
};

class SpacetimeKeypoint : public PosOrnKeypoint {  // SpacetimeKeypoint.h:15-45
public:
    SpacetimeKeypoint(const Vec& position, const Vec& orientation, const Mat& precision, const double& continuous_time, const int& timestep);
    SpacetimeKeypoint(const Vec& position, const Vec& dposition, const Vec& orientation, const Vec& dorientation, const Mat& precision,
                      const double& continuous_time, const int& timestep);
    double getContinuousTime() { return continuous_time_; }
    Vec diff(const Vec& state) const override;
    Vec getState() const override;
    Vec targetFx() const override;

protected:
    double continuous_time_;
};

class System {  // System.h:28-194
public:
    System(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
           const Vec& qMax, const Vec& qMin, const Vec& dqMax, const Vec& dqMin, int horizon, int nb_deriv, const std::vector<std::string>& tags);
    System(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
           int horizon, int nb_deriv, const std::vector<std::string>& tags);
    virtual ~System() {}
    virtual Vec getMuVector(bool sparse);
    virtual Mat getQMatrix(bool sparse);
    Mat getRt();
    int getNbStateVar() { return nb_state_var_; }
    int getNbCtrlVar() { return nb_ctrl_var_; }
    int getNbTargetVar() { return nb_target_var_; }
    int getNbQVar() { return nb_Q_var_; }
    int getHorizon() { return horizon_; }
    std::vector<int> getKpIndexes();
    Vec getInitState() { return x0_; }
    Vec getInitFoXState() { return f_x0_; }
    virtual Vec getState() = 0;
    virtual void reset() = 0;
    // ---- single-point evaluation API of System.h:66-194 (host glue over the simulator, whose kinematics run on the device).
    // The solvers never call these: they lower the system and run the batched kernels.
    typedef std::tuple<Vec, Vec, Mat, Mat, Mat> StepOut;                          // x, f(x), A, B, J
    typedef std::tuple<Vec, Vec, Vec, Vec, Mat, Mat, Mat, Mat> StepLimitsOut;     // x, f(x), q, u, A, B, J, L
    virtual StepOut forwardPass(const Vec& xk, const Vec& uk, int k) = 0;         // advances the simulator (xk is ignored as upstream)
    virtual std::tuple<Vec, Mat> getFxJac() = 0;
    virtual std::tuple<Vec, Mat> getFxJac(const Vec& xk);                         // System.cpp:163-179
    virtual Vec diff(const Vec& actual_state, int k);                             // :103-109
    Vec diffBatch(const Vec& x);                                                  // :111-119
    std::pair<Mat, Vec> inspectJointLimit(const Vec& xk);                         // :121-142
    StepLimitsOut forwardPassWithLimits(const Vec& xk, const Vec& uk, int k);     // :144-161
    std::tuple<Vec, Vec, std::vector<std::tuple<Mat, Mat, Mat, Mat>>> fpBatch(const Vec& u);  // :181-211
    virtual Vec cost(const Vec& xk, const Vec& uk, int k);                        // :213-234
    virtual Vec cost_x(const Vec& xk, const Vec& uk, int k);                      // :248-272
    virtual Mat cost_xx(const Vec& xk, const Vec& uk, int k);                     // :286-308
    Vec cost_u(const Vec&, const Vec& uk, int) { Vec o(uk.size()); for (size_t i = 0; i < uk.size(); i++) o[i] = Rdiag[i] * uk[i]; return o; }
    Mat cost_uu(const Vec&, const Vec&, int) { return getRt(); }
    Mat cost_ux(const Vec&, const Vec& uk, int) { return Mat((int)uk.size(), nb_state_var_); }
    Mat cost_xu(const Vec&, const Vec& uk, int) { return Mat(nb_state_var_, (int)uk.size()); }
    virtual Vec cost_F(const Vec& xk) { return cost(xk, Vec(nb_ctrl_var_, 0.0), horizon_ - 1); }
    virtual Vec cost_F_x(const Vec& xk) { return cost_x(xk, Vec(nb_ctrl_var_, 0.0), horizon_ - 1); }
    virtual Mat cost_F_xx(const Vec& xk) { return cost_xx(xk, Vec(nb_ctrl_var_, 0.0), horizon_ - 1); }
    std::shared_ptr<Keypoint> getKeypoint(int k) const;                           // :96-101 (the last of duplicates wins, as in the map)
    std::shared_ptr<sim::SimulationInterface> robot() { return r; }
    const std::vector<std::shared_ptr<Keypoint>>& getKeypoints() const { return keypoints; }
    // Lowering to the C ABI's POD descriptor.  Throws for systems the device cannot run.
    virtual void lower(ilqr_problem_desc* d) const;
    // Indices into getKeypoints() of the descriptor's keypoints, in descriptor order: of the keypoints given for one timestep a plain System
    // keeps the last (the map of System::init, System.cpp:78-80); a SequentialSystem keeps each sub-system's and orders a shared step's
    // keypoints by sub-system index.
    virtual std::vector<int> deviceKeypoints() const;
    // some timestep holds more than one keypoint of getKeypoints() (the batch solvers refuse such systems)
    bool hasSharedStep() const;
    virtual bool builtinType() const { return false; }  // overridden by the classes of this header: typeid(*this) == typeid(<that class>)
    // per-instance pieces for B = 1: q0, dq0 captured by localInit
    Vec q0() const { return q0_; }
    Vec dq0() const { return dq0_; }
    int getNbDeriv() const { return nb_deriv_; }
    // true for the system classes of this header exactly as declared here (with built-in keypoints): the shapes the device descriptor
    // describes.  A user-defined subclass -- also one derived from a built-in class -- answers false and is solved over its virtuals by
    // ILQRRecursive::solve (ilqr_host_loop.cpp); the choice is made on the type, never on whether a device call succeeded.
    bool builtin() const;
    const Vec& Rt() const { return Rdiag; }
    int kind() const { return kind_; }

protected:
    void init();
    void checkKeypoints();
    std::shared_ptr<sim::SimulationInterface> r;
    std::vector<std::shared_ptr<Keypoint>> keypoints;
    Vec Rdiag;
    Vec state_max_, state_min_;
    std::vector<int> joint_limits_weight_;
    Vec q0_, dq0_, x0_, f_x0_;
    int horizon_, nb_deriv_;
    int nb_state_var_ = 0, nb_ctrl_var_ = 0, nb_target_var_ = 0, nb_Q_var_ = 0;
    double penalty_ = 0, dt_ = 0;
    bool limits_set_ = false;
    int kind_ = ILQR_SYS_POS_ORN;
    std::vector<std::string> EXPECTED_KP_TAGS_;
};

class PosOrnPlannerSys : public System {  // PosOrnPlannerSys.h
public:
    bool builtinType() const override { return typeid(*this) == typeid(PosOrnPlannerSys); }
    PosOrnPlannerSys(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
                     const Vec& qMax, const Vec& qMin, const Vec& dqMax, const Vec& dqMin, int horizon, int nb_deriv, double dt);
    PosOrnPlannerSys(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
                     const Vec& qMax, const Vec& qMin, int horizon, int nb_deriv, double dt);
    PosOrnPlannerSys(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
                     int horizon, int nb_deriv, double dt);
    Vec getState() override;
    void reset() override;
    StepOut forwardPass(const Vec& xk, const Vec& uk, int k) override;
    std::tuple<Vec, Mat> getFxJac() override;
    using System::getFxJac;

protected:
    void localInit(double dt);
};

// Target space = joint space, J = I (JointSpacePlannerSys.h / .cpp:50-122).  Device path: nb_deriv = 1 (the reference's 2nd-order variant is
// dimensionally inconsistent) and 1 to 7 joints (the C ABI widens a shorter chain to the 7 the kernels are built for).
class JointSpacePlannerSys : public System {
public:
    bool builtinType() const override { return typeid(*this) == typeid(JointSpacePlannerSys); }
    JointSpacePlannerSys(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
                         const Vec& qMax, const Vec& qMin, const Vec& dqMax, const Vec& dqMin, int horizon, int nb_deriv, double dt);
    JointSpacePlannerSys(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
                         const Vec& qMax, const Vec& qMin, int horizon, int nb_deriv, double dt);
    JointSpacePlannerSys(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
                         int horizon, int nb_deriv, double dt);
    Vec getState() override;
    void reset() override;
    StepOut forwardPass(const Vec& xk, const Vec& uk, int k) override;
    std::tuple<Vec, Mat> getFxJac() override;
    using System::getFxJac;
    void lower(ilqr_problem_desc* d) const override;

protected:
    void localInit(double dt);
};

// JointSpacePlannerSys with a time state and dt = u_last^2 (JointSpaceTimePlannerSys.h / .cpp:50-160); nb_deriv = 1, 1 to 7 joints (widened
// to 7 by the C ABI)
class JointSpaceTimePlannerSys : public System {
public:
    bool builtinType() const override { return typeid(*this) == typeid(JointSpaceTimePlannerSys); }
    JointSpaceTimePlannerSys(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
                             const Vec& qMax, const Vec& qMin, const Vec& dqMax, const Vec& dqMin, int horizon, int nb_deriv);
    JointSpaceTimePlannerSys(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
                             const Vec& qMax, const Vec& qMin, int horizon, int nb_deriv);
    JointSpaceTimePlannerSys(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
                             int horizon, int nb_deriv);
    Vec getState() override;
    void reset() override;
    StepOut forwardPass(const Vec& xk, const Vec& uk, int k) override;
    std::tuple<Vec, Mat> getFxJac() override;
    std::tuple<Vec, Mat> getFxJac(const Vec& xk) override;
    void lower(ilqr_problem_desc* d) const override;

protected:
    void localInit();
};

class PosOrnTimePlannerSys : public System {  // PosOrnTimePlannerSys.h
public:
    bool builtinType() const override { return typeid(*this) == typeid(PosOrnTimePlannerSys); }
    PosOrnTimePlannerSys(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
                         const Vec& qMax, const Vec& qMin, const Vec& dqMax, const Vec& dqMin, int horizon, int nb_deriv);
    PosOrnTimePlannerSys(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
                         const Vec& qMax, const Vec& qMin, int horizon, int nb_deriv);
    PosOrnTimePlannerSys(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<Keypoint>>& keypoints, const Vec& RtDiag,
                         int horizon, int nb_deriv);
    Vec getState() override;
    void reset() override;
    StepOut forwardPass(const Vec& xk, const Vec& uk, int k) override;
    std::tuple<Vec, Mat> getFxJac() override;
    std::tuple<Vec, Mat> getFxJac(const Vec& xk) override;

protected:
    void localInit();
};
// Sum of the costs of several Systems sharing one robot (SequentialSystem.h / .cpp:20-168): dynamics of the first, keypoints of
// all (each in its own sub-system's frame, with that sub-system's control penalty), limit terms once per sub-system.
class SequentialSystem : public System {
public:
    bool builtinType() const override;  // ... and every sub-system is
    SequentialSystem(const std::shared_ptr<sim::SimulationInterface>& r, const std::vector<std::shared_ptr<System>>& systems, const Vec& RtDiag,
                     int horizon, int nb_deriv);
    Vec getState() override { return systems_.at(0)->getState(); }
    void reset() override;
    StepOut forwardPass(const Vec& xk, const Vec& uk, int k) override;
    std::tuple<Vec, Mat> getFxJac() override;
    using System::getFxJac;
    Vec diff(const Vec& state, int k) override;                       // SequentialSystem.cpp:167-183
    Vec cost(const Vec& xk, const Vec& uk, int k) override;           // :143-149 (sums of the sub-systems, as are the five below)
    Vec cost_x(const Vec& xk, const Vec& uk, int k) override;
    Mat cost_xx(const Vec& xk, const Vec& uk, int k) override;
    Vec cost_F(const Vec& xk) override;
    Vec cost_F_x(const Vec& xk) override;
    Mat cost_F_xx(const Vec& xk) override;
    Vec getMuVector(bool sparse) override;                            // :185-226
    Mat getQMatrix(bool sparse) override;                             // :228-274 (block diagonals of the sub-systems)
    void lower(ilqr_problem_desc* d) const override;
    std::vector<int> deviceKeypoints() const override;
    const std::vector<std::shared_ptr<System>>& systems() const { return systems_; }

protected:
    std::vector<std::shared_ptr<System>> systems_;
};
}  // namespace sys

namespace solver {

// Result of a batched solve: instance b is what the reference's solve() would have returned for that instance.
struct BatchResult {
    int B = 0, T = 0, n_x = 0, n_u = 0, n_f = 0;
    std::vector<double> X, fX, U, K, d;  // [B][T][n_x], [B][T][n_f], [B][T-1][n_u], [B][T-1][n_u][n_x], [B][T-1][n_u]
    std::vector<double> cost, alpha;     // [B]
    std::vector<int> iters, status;      // [B]
    std::vector<double> cost_trace, alpha_trace;  // [B][nb_iter]
    int nb_iter = 0;
    double seconds = 0;
};

// Clearance (include/ilqr_hip.h "clearance"): the robot as spheres on the links of the system's chain, the cell as half-spaces, the obstacles
// as spheres in sets.  Judged at the states of a trajectory by the clearance calls; with a weight (BatchInputs::obstacle_weight, MultiStartInputs::obstacle_weight)
// the same description is the obstacle term of the Riccati solvers' stage cost (include/ilqr_hip.h "obstacle terms").
struct ClearanceInputs {
    std::vector<int> sph_link;        // [n_sph], non-decreasing: -1 the base, s the frame behind segment s of the chain
    std::vector<double> sph_c, sph_r; // [n_sph][3] in the link's frame, [n_sph]
    std::vector<double> plane_n, plane_d;   // [n_planes][3] unit normals, [n_planes]: n . p >= d
    std::vector<double> obstacles;    // [n_sets][n_obs][4] = (cx, cy, cz, R), R < 0: unused slot
    std::vector<int> self_pairs;      // [n_self][2] = (a, b): two of the robot's own spheres, a < b on different links (ilqr_clr_robot::self_pair)
    int n_sets = 0, n_obs = 0;
    double margin = 0;
    bool given() const { return !sph_link.empty(); }
};
// Per-instance inputs of a batched solve; anything left empty takes the System's own value for every instance.
struct BatchInputs {
    int B = 1;
    std::vector<double> q0, dq0;                    // [B][dof]
    std::vector<std::vector<double>> kp_targets;    // per keypoint: [B][n_f] in f(x) order
    std::vector<double> U0;                         // [B][T-1][n_u]  (or [T-1][n_u], broadcast)
    bool want_fX = true, want_gains = true;
    // K, d of the result are the gains about the plan the solve leaves (ilqr_problem_gains: one sweep about the returned X, U, feed-forward
    // unscaled), for any solver -- the batch solvers, which leave none of their own, included; the closed loops then run on them
    bool plan_gains = false;
    // AL_ILQR only (the other classes throw if it is set): positive = K, d of the result are the gains about the plan WITH the augmented-
    // Lagrangian terms of the lowered rows at this penalty (ilqr_problem_gains_al: active-set weights of the plan, the multipliers the solve
    // leaves); it implies plan_gains, and closedLoopBatch / closedLoopCovBatch run on them.  0 = off.  AL_ILQR::finalPenalty gives the
    // penalty a solve ends with.
    double al_gains_penalty = 0;
    // ILQRRecursive and AL_ILQR: obstacle_weight > 0 with spheres given adds the obstacle terms to the stage cost (ilqr_problem_set_obstacles with
    // obstacles.margin as the activation distance): obstacles [n_sets][n_obs][4] with B % n_sets == 0, instance b reads set b / (B / n_sets).
    // Such a solve runs on the generic kernels unless obstacle_path asks for the cooperative ones.  0 = off: the solve is exactly what it is without these fields.
    ClearanceInputs obstacles;
    double obstacle_weight = 0;
    int obstacle_path = 0;   // ILQR_OBSTACLE_PATH_* for this call (solveBatch / solveMultiStart): set on the context before the solves, the previous mode restored after
};

// Multi-start (include/ilqr_hip.h "multi-start"): every task of a BatchInputs (in.B = G tasks) is solved from S starts on G * S instances --
// member 0 from the task's own U0, the others from U0 + sigma_u z (ilqr_problem_spread_controls) -- for coarse_iter iterations; the start with
// the lowest cost wins its group (ilqr_problem_select), and its plan is polished by the caller's nb_iter iterations on the G problem.
struct ClearanceResult {
    int n = 0, T = 0, n_groups = 0;
    std::vector<double> clr, clr_min, stats;        // [n][T], [n], [n_groups][ILQR_CLR_STATS] (empty without stats_group)
    std::vector<int> clr_at, n_below, eligible;     // [n][3], [n], [n]
};
// ilqr_clearance_trajectories on X[n][T][n_x] in the layout of the system: traj_per_set trajectories share a set of obstacles (0: all of them),
// stats_group > 0 asks for the per-group stats
ClearanceResult clearance(sys::System& s, const std::vector<double>& X, int n, int T, const ClearanceInputs& c, int traj_per_set = 0, int stats_group = 0);

struct MultiStartInputs {
    int S = 1;                      // starts per task
    unsigned long long seed = 0;
    std::vector<double> sigma_u;    // one value (every control entry) or n_u values in the user's layout; empty: 0
    int coarse_iter = 1;            // iterations every start runs before the selection
    // given: obstacles[G][n_obs][4], one set per task.  The starts are scored after the coarse solves (ilqr_problem_clearance, traj_per_set = S)
    // and only those with clearance >= margin are candidates of the selection; the polished plans are scored again.  A filter, not avoidance.
    ClearanceInputs clearance;
    // > 0 (needs `clearance`): the same spheres, planes and obstacles are also obstacle terms of both solves' stage cost, with clearance.margin as
    // the activation distance -- on the starts (traj_per_set = S) and on the tasks (1).  The filter and the reported clearances stay as they are.
    // 0 = off: exactly the call without it.
    double obstacle_weight = 0;
};
// The usual result of the G tasks (the polished plans; cost_trace / alpha_trace are the polishing solve's) and what the selection saw
struct MultiStartResult : BatchResult {
    int S = 0;
    std::vector<int> winner, n_candidates;           // [G]: the winning instance g * S + s, the number of candidates of the group
    std::vector<double> coarse_best, coarse_first;   // [G]: the winner's cost after the coarse iterations, member 0's
    // with MultiStartInputs::clearance (else empty): the winner's clearance after the coarse iterations -- negative or below the margin where its
    // group had no eligible start (winner = member 0, n_candidates = 0) -- and clr_min, clr_at, n_below of the polished plans
    std::vector<double> coarse_clearance, clearance;   // [G]
    std::vector<int> clearance_at, n_below;            // [G][3], [G]
};
struct MultiStartOut;   // ilqr_host.cpp

// Closed loop of the tracking law on the plan a batched Riccati solve leaves (ilqr_problem_closed_loop): S executions per instance.
struct ClosedLoopInputs {
    int S = 1;
    std::vector<double> x0;   // [B][S][n_x] or empty: every execution starts on the plan
    std::vector<double> w;    // [B][S][T-1][n_x] or empty: no disturbance
    bool with_feedforward = false;
    // seed given: the disturbances sigma_w z and the start perturbations sigma_x0 z are drawn on the device (ilqr_problem_closed_loop_noise);
    // x0 is then the centre of the start perturbation and w must be empty
    bool has_seed = false;
    unsigned long long seed = 0;
    std::vector<double> sigma_w, sigma_x0;   // one value (every entry) or n_x values; empty: 0
    // tolerances given: the executions are also reported on (ilqr_problem_closed_loop_report, the definitions of include/ilqr_hip.h)
    bool has_tol = false;
    std::vector<double> kp_tol;   // one value (every keypoint and group), ILQR_KP_ERR values (every keypoint) or n_kp x ILQR_KP_ERR; negative: not
                                  // judged; empty: nothing is judged
    double lim_tol = 0;
    // con_tol given (AL_ILQR): the executions are also judged against the constraint rows the class lowers (ilqr_problem_closed_loop_report_con)
    bool has_con_tol = false;
    double con_tol = 0;
};
struct ClosedLoopResult {
    int B = 0, S = 0, T = 0, n_x = 0, n_u = 0;
    std::vector<double> cost, X, U;  // [B][S], [B][S][T][n_x], [B][S][T-1][n_u]
    std::vector<double> stats;       // [B][5]: mean, unbiased variance, min, max of the finite costs in sample order, and the number that are not finite
    // with tolerances (ClosedLoopInputs::has_tol), else empty: [B][S][n_kp][5], [B][n_kp][12], [B][S], [B][4]
    int n_kp = 0;
    std::vector<double> kp_err, kp_stats, lim_cost, outcome;
    // with con_tol (ClosedLoopInputs::has_con_tol), else empty: [B][S], [B][S], [B][6]; outcome_con [B][5] with tolerances as well
    std::vector<double> con_max, con_steps, con_stats, outcome_con;
};

// The covariance of that closed loop under the noise model of ClosedLoopInputs::seed, propagated analytically (ilqr_problem_closed_loop_cov)
struct ClosedLoopCovInputs {
    std::vector<double> sigma_w, sigma_x0;   // one value (every entry) or n_x values; empty: 0
    bool want_Sigma = false;                 // the covariance at every step (B T n_x^2 doubles)
    bool want_con = false;                   // AL_ILQR: the variance of the constraint rows the class lowers (ilqr_problem_closed_loop_cov_con)
    // given: the clearance pairs of the plans under the covariance (ilqr_problem_closed_loop_cov_clr): obstacles [n_sets][n_obs][4] with
    // B % n_sets == 0, instance b reads set b / (B / n_sets); clearance.margin is the margin of z, z_tol the bound of `eligible`
    ClearanceInputs clearance;
    double z_tol = 0;
};
// the one place of closed_loop_cov_batch's rule for a sigma (a scalar or nb_state_var entries) and of its error text, which is closed_loop_batch's
[[noreturn]] void closed_loop_cov_sigma_error();
struct ClosedLoopCovResult {
    int B = 0, T = 0, n_x = 0, n_u = 0, n_kp = 0;
    std::vector<double> Sigma;                           // [B][T][n_x][n_x], empty unless asked for
    std::vector<double> kp_Sigma, kp_var, u_var, lim_z;  // [B][n_kp][n_x][n_x], [B][n_kp][5], [B][T-1][n_u], [B]
    int m = 0;                                           // the rows the class lowered
    std::vector<double> con_var, con_z;                  // [B][T-1][m], [B]; empty unless want_con
    std::vector<double> clr_var, clr_z, clr_z_min;       // [B][T], [B][T], [B]; empty unless ClosedLoopCovInputs::clearance is given
    std::vector<int> clr_z_at, eligible;                 // [B][3], [B]; likewise
};

struct Constraint {  // AL-ILQR.h:20-23
    Mat A;
    Vec b;
};

// ILQRRecursive over the virtual interface of a user-defined system (ilqr_host_loop.cpp)
std::tuple<std::vector<Vec>, std::vector<Vec>, std::vector<Vec>, std::vector<Mat>, std::vector<Vec>, double> solve_over_virtuals(
    sys::System& s, const std::vector<Vec>& U0, int nb_iter, bool line_search, bool early_stop, CallBackMessage* cb);

// AL_ILQR over the same interface (multipliers updated in place, as the reference's member is)
std::tuple<std::vector<Vec>, std::vector<Vec>, std::vector<Vec>> solve_al_over_virtuals(sys::System& s, const std::vector<Constraint>& inequality, std::vector<Vec>& multipliers,
                                                                                        const std::vector<Vec>& U0, int nb_iter, int lag_update_step, double penalty,
                                                                                        double scaling_factor, bool line_search, bool early_stop, CallBackMessage* cb);

// BatchILQR (psi = nullptr) / BatchILQRCP over the same interface: one Gauss-Newton step on the whole control sequence per iteration
Vec solve_batch_over_virtuals(sys::System& s, const Mat* psi, const Mat& Q, int nb_iter, const Vec& u0, bool early_stop, CallBackMessage* cb);

class ILQRRecursive {  // ILQRRecursive.h:21-42
public:
    explicit ILQRRecursive(const std::shared_ptr<sys::System>& s) : s(s) {}
    std::tuple<std::vector<Vec>, std::vector<Vec>, std::vector<Vec>, std::vector<Mat>, std::vector<Vec>, double> solve(
        const std::vector<Vec>& U0, int nb_iter, bool line_search = true, bool early_stop = true, CallBackMessage* cb = nullptr);
    BatchResult solveBatch(const BatchInputs& in, int nb_iter, bool line_search = true, bool early_stop = true);
    // every task from ms.S starts: adopt, spread_controls, ms.coarse_iter iterations, select by cost, adopt the winners' controls, nb_iter iterations
    MultiStartResult solveMultiStart(const BatchInputs& in, const MultiStartInputs& ms, int nb_iter, bool line_search = true, bool early_stop = true);
    // solveBatch, then the closed loop on its plan, in one stateless call
    std::pair<BatchResult, ClosedLoopResult> closedLoopBatch(const BatchInputs& in, const ClosedLoopInputs& cl, int nb_iter, bool line_search = true,
                                                             bool early_stop = true);
    // solveBatch, then the analytic covariance of the closed loop on its plan
    std::pair<BatchResult, ClosedLoopCovResult> closedLoopCovBatch(const BatchInputs& in, const ClosedLoopCovInputs& cv, int nb_iter, bool line_search = true,
                                                                   bool early_stop = true);

private:
    std::shared_ptr<sys::System> s;
};

class AL_ILQR {  // AL-ILQR.h:25-72
public:
    AL_ILQR(const std::shared_ptr<sys::System>& s, const std::vector<Constraint>& inequality, const std::vector<Vec>& initLambda);
    std::tuple<std::vector<Vec>, std::vector<Vec>, std::vector<Vec>> solve(const std::vector<Vec>& U0, int nb_iter, int lag_update_step, double penalty,
                                                                          double scaling_factor, bool line_search = true, bool early_stop = false,
                                                                          CallBackMessage* cb = nullptr);
    BatchResult solveBatch(const BatchInputs& in, int nb_iter, int lag_update_step, double penalty, double scaling_factor, bool line_search = true,
                           bool early_stop = false);
    std::pair<BatchResult, ClosedLoopResult> closedLoopBatch(const BatchInputs& in, const ClosedLoopInputs& cl, int nb_iter, int lag_update_step, double penalty,
                                                             double scaling_factor, bool line_search = true, bool early_stop = false);
    std::pair<BatchResult, ClosedLoopCovResult> closedLoopCovBatch(const BatchInputs& in, const ClosedLoopCovInputs& cv, int nb_iter, int lag_update_step,
                                                                   double penalty, double scaling_factor, bool line_search = true, bool early_stop = false);
    // as ILQRRecursive::solveMultiStart; the winners' multipliers are adopted with their controls, and the nb_iter iterations start from
    // finalPenalty(ms.coarse_iter, ..)
    MultiStartResult solveMultiStart(const BatchInputs& in, const MultiStartInputs& ms, int nb_iter, int lag_update_step, double penalty, double scaling_factor,
                                     bool line_search = true, bool early_stop = false);
    // the penalty a solve of nb_iter iterations ends with: penalty *= scaling_factor once per update iteration ((it + 1) % lag_update_step == 0),
    // formed as the solver forms it (the same double) -- what BatchInputs::al_gains_penalty wants for the gains about that solve's plan
    static double finalPenalty(int nb_iter, int lag_update_step, double penalty, double scaling_factor);

private:
    BatchResult solveBatchThen(const BatchInputs& in, int nb_iter, int lag_update_step, double penalty, double scaling_factor, bool line_search, bool early_stop,
                               const std::function<void(ilqr_problem*)>& then, const MultiStartInputs* ms = nullptr, MultiStartOut* mo = nullptr);
    std::shared_ptr<sys::System> s;
    std::vector<Constraint> inequality;
    std::vector<Vec> multipliers;  // persists across solve() calls like the reference's member
    int lowered_m = 0;             // rows of the last solveBatchThen on the device (the all-zero ones are dropped)
};

class BatchILQR {  // BatchILQR.h:21-53: the batch solver on the full control sequence (= BatchILQRCP with the identity basis)
public:
    BatchILQR(const std::shared_ptr<sys::System>& s, const Mat& Q);
    explicit BatchILQR(const std::shared_ptr<sys::System>& s);
    Vec solve(int nb_iter, const Vec& u0, bool early_stop = true, CallBackMessage* cb = nullptr);
    BatchResult solveBatch(const BatchInputs& in, int nb_iter, bool early_stop = true);
    // solveBatch, the gains about its plan (ilqr_problem_gains), then the closed loop / its analytic covariance on them
    std::pair<BatchResult, ClosedLoopResult> closedLoopBatch(const BatchInputs& in, const ClosedLoopInputs& cl, int nb_iter, bool early_stop = true);
    std::pair<BatchResult, ClosedLoopCovResult> closedLoopCovBatch(const BatchInputs& in, const ClosedLoopCovInputs& cv, int nb_iter, bool early_stop = true);

private:
    std::shared_ptr<sys::System> s;
    Mat Q;  // only the block-diagonal of the keypoints' precisions is supported on the device
    bool custom_Q = false;
};

class BatchILQRCP {  // BatchILQRCP.h:21-52
public:
    BatchILQRCP(const std::shared_ptr<sys::System>& s, const Mat& Q, const Mat& psi);
    BatchILQRCP(const std::shared_ptr<sys::System>& s, const Mat& psi);
    Vec solve(int nb_iter, const Vec& u0, bool early_stop = true, CallBackMessage* cb = nullptr);
    BatchResult solveBatch(const BatchInputs& in, int nb_iter, bool early_stop = true);
    // solveBatch, the gains about its plan (ilqr_problem_gains), then the closed loop / its analytic covariance on them
    std::pair<BatchResult, ClosedLoopResult> closedLoopBatch(const BatchInputs& in, const ClosedLoopInputs& cl, int nb_iter, bool early_stop = true);
    std::pair<BatchResult, ClosedLoopCovResult> closedLoopCovBatch(const BatchInputs& in, const ClosedLoopCovInputs& cv, int nb_iter, bool early_stop = true);

private:
    std::shared_ptr<sys::System> s;
    Mat PSI;
    Mat Q;  // only the block-diagonal of the keypoints' precisions is supported on the device
    bool custom_Q = false;
};

class LQT {  // lqt.h:23-86: linear-quadratic tracking of the targets `states` (N = states.size() / n), R = pow(rfactor, nb_deriv) I
public:
    LQT(const Mat& A, const Mat& B, const std::vector<Mat>& Qs, const Vec& states, float rfactor = 0.1f, int nb_deriv = 2);
    void solveDP();     // terminal weight Qs.back(), Qs.at(t) before it
    void solveLinAl();  // Qs.at(0 .. N-1); x_0 = mu_0
    Vec getCommand(int timestep, const Vec& curr_state);  // after solveDP; timestep in -1 .. N-2, else std::out_of_range
    Vec getCommand(int timestep);                         // after solveLinAl; timestep in 0 .. N-2, else std::out_of_range (the reference
                                                          // does not check it)
    int getNbStates() const { return N; }
    Vec getPredictedStates();  // after solveLinAl: [N * n], x_0 = mu_0 first

private:
    std::shared_ptr<ilqr_lqt> upload(const std::vector<Mat>& Q) const;
    Mat A, B;
    std::vector<Mat> Qs;
    Vec mu;
    double r;
    int n, m, N;
    std::shared_ptr<ilqr_lqt> dp;  // the device handle of solveDP (getCommand(t, x) runs on it)
    Vec U, X;                      // solveLinAl's controls and predicted states
};
}  // namespace solver
}  // namespace ilqr_planner
