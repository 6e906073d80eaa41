// pylqr_bindings.cpp -- pybind11 module `PyLQR` with the reference's Python surface (pylqr_planner/src/bindings.cpp:48-908)
// for the classes the device hot path covers, plus the new `solve_batch` entry points.
// Same module / submodule / class / method / argument names; numpy in, numpy out (the reference's Eigen casters);
// no argument has a default, as in the reference.  Errors are std::runtime_error -> RuntimeError.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include "ilqr_host.hpp"

namespace py = pybind11;
using namespace ilqr_planner;
using arr_t = py::array_t<double, py::array::c_style | py::array::forcecast>;

// Vec <-> 1-D float64 ndarray, Mat <-> 2-D float64 ndarray (declared before <pybind11/stl.h> so they win over its list caster)
namespace pybind11 {
namespace detail {
template <>
struct type_caster<Vec> {
    PYBIND11_TYPE_CASTER(Vec, const_name("numpy.ndarray[float64[n]]"));
    bool load(handle src, bool) {
        if (!src || src.is_none()) return false;
        arr_t a = arr_t::ensure(src);
        if (!a) return false;
        value.assign(a.data(), a.data() + a.size());
        return true;
    }
    static handle cast(const Vec& v, return_value_policy, handle) {
        py::array_t<double> a((py::ssize_t)v.size());
        std::copy(v.begin(), v.end(), a.mutable_data());
        return a.release();
    }
};
template <>
struct type_caster<Mat> {
    PYBIND11_TYPE_CASTER(Mat, const_name("numpy.ndarray[float64[m, n]]"));
    bool load(handle src, bool) {
        if (!src || src.is_none()) return false;
        arr_t a = arr_t::ensure(src);
        if (!a || a.ndim() > 2) return false;
        if (a.ndim() == 2) value = Mat((int)a.shape(0), (int)a.shape(1));
        else value = Mat((int)a.size(), 1);
        std::copy(a.data(), a.data() + a.size(), value.d.begin());
        return true;
    }
    static handle cast(const Mat& m, return_value_policy, handle) {
        py::array_t<double> a({(py::ssize_t)m.rows, (py::ssize_t)m.cols});
        std::copy(m.d.begin(), m.d.end(), a.mutable_data());
        return a.release();
    }
};
}  // namespace detail
}  // namespace pybind11

#include <pybind11/stl.h>

class PythonCallbackMessage : public CallBackMessage {  // pylqr_planner/src/PythonCallbackMessage.cpp:14-17
public:
    void notify(const std::string& msg) override { py::print(msg); }
};

static py::array_t<double> shaped(const std::vector<double>& v, std::vector<py::ssize_t> shape) {
    py::array_t<double> a(shape);
    std::copy(v.begin(), v.end(), a.mutable_data());
    return a;
}
static py::array_t<int> shaped_i(const std::vector<int>& v, std::vector<py::ssize_t> shape) {
    py::array_t<int> a(shape);
    std::copy(v.begin(), v.end(), a.mutable_data());
    return a;
}

// solve_batch(..., plan_gains = True): K, d of the result are the gains about the plan the solve leaves (ilqr_problem_gains)
static solver::BatchInputs plan_gains(solver::BatchInputs in, bool on) {
    in.plan_gains = on;
    return in;
}

// AL_ILQR: al_gains_penalty = p: K, d are the gains about that plan with the AL terms of the lowered rows at penalty p (ilqr_problem_gains_al)
static solver::BatchInputs al_gains(solver::BatchInputs in, const py::object& penalty) {
    if (!penalty.is_none()) in.al_gains_penalty = penalty.cast<double>();
    return in;
}

// numpy -> BatchInputs: U0 [B][T-1][n_u] or [T-1][n_u]; q0/dq0 [B][dof] or None; kp_targets list of [B][n_f] or None
static solver::BatchInputs batch_inputs(const py::object& U0, const py::object& q0, const py::object& dq0, const py::object& kp_targets, bool flat_u = false) {
    solver::BatchInputs in;
    in.B = 1;
    arr_t u = arr_t::ensure(U0);
    if (!u) throw std::runtime_error("[solve_batch] U0 must be a float array");
    in.U0.assign(u.data(), u.data() + u.size());
    if (u.ndim() == 3 || (flat_u && u.ndim() == 2)) in.B = (int)u.shape(0);  // flat_u: [B][(T-1) n_u] (Batch-CP's vectorised u)
    if (!q0.is_none()) {
        arr_t a = arr_t::ensure(q0);
        if (!a || a.ndim() != 2) throw std::runtime_error("[solve_batch] q0 must be B x dof");
        in.q0.assign(a.data(), a.data() + a.size());
        in.B = (int)a.shape(0);
    }
    if (!dq0.is_none()) {
        arr_t a = arr_t::ensure(dq0);
        if (!a || a.ndim() != 2) throw std::runtime_error("[solve_batch] dq0 must be B x dof");
        in.dq0.assign(a.data(), a.data() + a.size());
    }
    if (!kp_targets.is_none()) {
        for (auto h : kp_targets.cast<py::list>()) {
            arr_t a = arr_t::ensure(py::reinterpret_borrow<py::object>(h));
            if (!a || a.ndim() != 2) throw std::runtime_error("[solve_batch] every kp_targets entry must be B x nb_target_var");
            in.kp_targets.emplace_back(a.data(), a.data() + a.size());
            in.B = (int)a.shape(0);
        }
    }
    return in;
}

// spheres: [(link, (cx, cy, cz), r), ...] in chain order; planes: [((nx, ny, nz), d), ...] or None; obstacles: [n_sets][n_obs][4] or None;
// self_pairs: [(a, b), ...] sphere indices or None
static solver::ClearanceInputs clearance_inputs(const py::object& spheres, const py::object& planes, const py::object& obstacles, double margin,
                                                const py::object& self_pairs = py::none()) {
    solver::ClearanceInputs c;
    c.margin = margin;
    if (spheres.is_none()) {
        if (!planes.is_none() || !obstacles.is_none() || !self_pairs.is_none()) throw std::runtime_error("[clearance] planes, obstacles and self pairs need the robot's spheres");
        return c;
    }
    if (!self_pairs.is_none())
        for (auto h : self_pairs.cast<py::list>()) {
            py::tuple t = py::reinterpret_borrow<py::object>(h).cast<py::tuple>();
            if (t.size() != 2) throw std::runtime_error("[clearance] a self pair is (a, b)");
            c.self_pairs.push_back(t[0].cast<int>());
            c.self_pairs.push_back(t[1].cast<int>());
        }
    for (auto h : spheres.cast<py::list>()) {
        py::tuple t = py::reinterpret_borrow<py::object>(h).cast<py::tuple>();
        if (t.size() != 3) throw std::runtime_error("[clearance] a sphere is (link, (cx, cy, cz), r)");
        c.sph_link.push_back(t[0].cast<int>());
        arr_t ctr = arr_t::ensure(t[1]);
        if (!ctr || ctr.size() != 3) throw std::runtime_error("[clearance] a sphere's centre has 3 entries");
        c.sph_c.insert(c.sph_c.end(), ctr.data(), ctr.data() + 3);
        c.sph_r.push_back(t[2].cast<double>());
    }
    if (!planes.is_none())
        for (auto h : planes.cast<py::list>()) {
            py::tuple t = py::reinterpret_borrow<py::object>(h).cast<py::tuple>();
            if (t.size() != 2) throw std::runtime_error("[clearance] a plane is ((nx, ny, nz), d)");
            arr_t nn = arr_t::ensure(t[0]);
            if (!nn || nn.size() != 3) throw std::runtime_error("[clearance] a plane's normal has 3 entries");
            c.plane_n.insert(c.plane_n.end(), nn.data(), nn.data() + 3);
            c.plane_d.push_back(t[1].cast<double>());
        }
    if (!obstacles.is_none()) {
        arr_t a = arr_t::ensure(obstacles);
        if (!a || a.ndim() != 3 || a.shape(2) != 4) throw std::runtime_error("[clearance] obstacles must be n_sets x n_obs x 4");
        c.n_sets = (int)a.shape(0);
        c.n_obs = (int)a.shape(1);
        c.obstacles.assign(a.data(), a.data() + a.size());
    }
    return c;
}

// solve_batch(..., spheres, planes, obstacles, margin, obstacle_weight): the obstacle terms of the stage cost (weight 0: none)
static solver::BatchInputs obstacle_terms(solver::BatchInputs in, const py::object& spheres, const py::object& planes, const py::object& obstacles, double margin,
                                          double weight, const py::object& self_pairs) {
    in.obstacles = clearance_inputs(spheres, planes, obstacles, margin, self_pairs);
    in.obstacle_weight = weight;
    if (weight != 0 && !in.obstacles.given()) throw std::runtime_error("[solve_batch] obstacle_weight needs the robot's spheres");
    return in;
}

// obstacle_path = "generic" | "cooperative" on solve_batch / solve_multistart: the kernel path of the call's obstacle terms (ILQR_OBSTACLE_PATH_*)
static solver::BatchInputs obstacle_path(solver::BatchInputs in, const std::string& path, const char* fn) {
    if (path == "generic") in.obstacle_path = 0;
    else if (path == "cooperative") in.obstacle_path = 1;
    else throw std::runtime_error(std::string("[") + fn + "] obstacle_path must be \"generic\" or \"cooperative\" (got \"" + path + "\")");
    return in;
}

// solve_multistart(..., S, seed, sigma_u, coarse_iter): sigma_u None (0), a scalar or nb_ctrl_var values
static solver::MultiStartInputs multistart_inputs(int S, unsigned long long seed, const py::object& sigma_u, int coarse_iter, const py::object& spheres = py::none(),
                                                  const py::object& planes = py::none(), const py::object& obstacles = py::none(), double margin = 0.0,
                                                  double obstacle_weight = 0.0, const py::object& self_pairs = py::none()) {
    solver::MultiStartInputs ms;
    ms.clearance = clearance_inputs(spheres, planes, obstacles, margin, self_pairs);
    ms.obstacle_weight = obstacle_weight;
    if (obstacle_weight != 0 && !ms.clearance.given()) throw std::runtime_error("[solve_multistart] obstacle_weight needs the robot's spheres");
    ms.S = S;
    ms.seed = seed;
    ms.coarse_iter = coarse_iter;
    if (!sigma_u.is_none()) {
        arr_t a = arr_t::ensure(sigma_u);
        if (!a || a.ndim() > 1) throw std::runtime_error("[solve_multistart] sigma_u must be a scalar or have nb_ctrl_var entries");
        ms.sigma_u.assign(a.data(), a.data() + a.size());
    }
    return ms;
}

// numpy -> ClosedLoopInputs: x0 [B][S][n_x] or None, w [B][S][T-1][n_x] or None; samples: S where neither array gives it
static solver::ClosedLoopInputs closed_loop_inputs(const py::object& x0, const py::object& w, const py::object& samples, bool with_ff,
                                                   const py::object& seed = py::none(), const py::object& sigma_w = py::none(),
                                                   const py::object& sigma_x0 = py::none(), const py::object& kp_tol = py::none(),
                                                   const py::object& lim_tol = py::none(), const py::object& con_tol = py::none()) {
    solver::ClosedLoopInputs cl;
    cl.with_feedforward = with_ff;
    if (!con_tol.is_none()) {
        cl.has_con_tol = true;
        cl.con_tol = con_tol.cast<double>();
    }
    if (!kp_tol.is_none() || !lim_tol.is_none()) {  // either one asks for the report
        cl.has_tol = true;
        if (!kp_tol.is_none()) {
            arr_t a = arr_t::ensure(kp_tol);
            if (!a || a.ndim() > 2) throw std::runtime_error("[closed_loop_batch] kp_tol must be a scalar, have 5 entries or be nb_keypoints x 5");
            cl.kp_tol.assign(a.data(), a.data() + a.size());
        }
        cl.lim_tol = lim_tol.is_none() ? 0.0 : lim_tol.cast<double>();
    }
    if (!seed.is_none()) {
        cl.has_seed = true;
        cl.seed = seed.cast<unsigned long long>();
        for (int which = 0; which < 2; which++) {
            const py::object& sg = which ? sigma_x0 : sigma_w;
            if (sg.is_none()) continue;
            arr_t a = arr_t::ensure(sg);
            if (!a || a.ndim() > 1) throw std::runtime_error("[closed_loop_batch] sigma_w and sigma_x0 must be a scalar or have nb_state_var entries");
            (which ? cl.sigma_x0 : cl.sigma_w).assign(a.data(), a.data() + a.size());
        }
    } else if (!sigma_w.is_none() || !sigma_x0.is_none()) throw std::runtime_error("[closed_loop_batch] sigma_w and sigma_x0 need a seed");
    int S = samples.is_none() ? -1 : samples.cast<int>();
    if (!x0.is_none()) {
        arr_t a = arr_t::ensure(x0);
        if (!a || a.ndim() != 3) throw std::runtime_error("[closed_loop_batch] x0 must be B x S x nb_state_var");
        cl.x0.assign(a.data(), a.data() + a.size());
        if (S < 0) S = (int)a.shape(1);
    }
    if (!w.is_none()) {
        arr_t a = arr_t::ensure(w);
        if (!a || a.ndim() != 4) throw std::runtime_error("[closed_loop_batch] w must be B x S x (horizon-1) x nb_state_var");
        cl.w.assign(a.data(), a.data() + a.size());
        if (S < 0) S = (int)a.shape(1);
    }
    cl.S = S < 0 ? 1 : S;
    return cl;
}

// numpy -> ClosedLoopCovInputs: a sigma is None, a scalar or nb_state_var entries
static solver::ClosedLoopCovInputs closed_loop_cov_inputs(const py::object& sigma_w, const py::object& sigma_x0, bool want_Sigma, bool want_con = false) {
    solver::ClosedLoopCovInputs cv;
    cv.want_Sigma = want_Sigma;
    cv.want_con = want_con;
    for (int which = 0; which < 2; which++) {
        const py::object& sg = which ? sigma_x0 : sigma_w;
        if (sg.is_none()) continue;
        arr_t a = arr_t::ensure(sg);
        if (!a || a.ndim() > 1) solver::closed_loop_cov_sigma_error();   // (the length is checked where nb_state_var is known)
        (which ? cv.sigma_x0 : cv.sigma_w).assign(a.data(), a.data() + a.size());
    }
    return cv;
}

// closed_loop_cov_batch(..., spheres, planes, obstacles, self_pairs, margin, z_tol): the clearance pairs under the covariance
// (ilqr_problem_closed_loop_cov_clr); without spheres the call is what it was
static solver::ClosedLoopCovInputs cov_clearance(solver::ClosedLoopCovInputs cv, const py::object& spheres, const py::object& planes, const py::object& obstacles,
                                                 const py::object& self_pairs, double margin, double z_tol) {
    cv.clearance = clearance_inputs(spheres, planes, obstacles, margin, self_pairs);
    cv.z_tol = z_tol;
    return cv;
}

PYBIND11_MODULE(PyLQR, m) {
    m.doc() = "PyLQR: the reference's Python surface over the MI355X-native batched iLQR hot path (libilqr_hip.so)";

    // ------------------------------------------------------------------ sim
    py::module m_sim = m.def_submodule("sim");
    py::class_<sim::SimulationInterface, std::shared_ptr<sim::SimulationInterface>>(m_sim, "SimulationInterface")
        .def("update_kinematics", &sim::SimulationInterface::updateKinematics)
        .def("Jt", &sim::SimulationInterface::Jt)
        .def("Jr", &sim::SimulationInterface::Jr)
        .def("J", &sim::SimulationInterface::J)
        .def("Jtp", &sim::SimulationInterface::Jtp)
        .def("Jrp", &sim::SimulationInterface::Jrp)
        .def("Jp", &sim::SimulationInterface::Jp)
        .def("get_ee_pos", &sim::SimulationInterface::getEEPosition)
        .def("get_ee_orn", &sim::SimulationInterface::getEEOrnQuat)
        .def("get_ee_vel", &sim::SimulationInterface::getEEVelocity)
        .def("get_ee_ang_vel", &sim::SimulationInterface::getEEAngVel)
        .def("get_ee_ang_vel_quat", &sim::SimulationInterface::getEEAngVelQuat)
        .def("get_q", &sim::SimulationInterface::getJointsPos)
        .def("get_dq", &sim::SimulationInterface::getJointsVel)
        .def("get_time", &sim::SimulationInterface::getTime)
        .def("set_time", &sim::SimulationInterface::setTime, py::arg("time"))
        .def("dquat_to_w_jac", &sim::SimulationInterface::dQuatToDxJac, py::arg("quat"))
        .def("set_conf", &sim::SimulationInterface::setConfiguration, py::arg("q"), py::arg("dq"), py::arg("reset_time"))
        .def("send_acc", &sim::SimulationInterface::sendAcc, py::arg("dt"), py::arg("ddq"), py::arg("updateKin"))
        .def("send_vel", &sim::SimulationInterface::sendVel, py::arg("dt"), py::arg("dq"), py::arg("updateKin"));
    py::class_<sim::KDLRobot, sim::SimulationInterface, std::shared_ptr<sim::KDLRobot>>(m_sim, "KDLRobot")
        .def(py::init<const std::string&, const std::string&, const std::string&, const Vec&, const Vec&, const Vec&, const Vec&, const bool&>(),
             py::arg("urdf"), py::arg("base_frame"), py::arg("tip_frame"), py::arg("q"), py::arg("dq"), py::arg("transform_rpy"), py::arg("transform_xyz"),
             py::arg("is_path"))
        .def(py::init<const std::string&, const std::string&, const std::string&, const Vec&, const Vec&, const Vec&, const Vec&>(), py::arg("urdf"),
             py::arg("base_frame"), py::arg("tip_frame"), py::arg("q"), py::arg("dq"), py::arg("transform_rpy"), py::arg("transform_xyz"))
        .def(py::init<const std::string&, const std::string&, const std::string&, const Vec&, const Vec&>(), py::arg("urdf"), py::arg("base_frame"),
             py::arg("tip_frame"), py::arg("q"), py::arg("dq"))
        .def("joint_lower_limits", &sim::KDLRobot::jointLowerLimits)
        .def("joint_upper_limits", &sim::KDLRobot::jointUpperLimits);
    // bindings.cpp:192-195
    py::class_<sim::Robot2D, sim::SimulationInterface, std::shared_ptr<sim::Robot2D>>(m_sim, "Robot2D")
        .def(py::init<const Vec&, const Vec&>(), py::arg("lengths"), py::arg("default_q"))
        .def("fkine", static_cast<Vec (sim::Robot2D::*)()>(&sim::Robot2D::fkine))
        .def("fkine", static_cast<Vec (sim::Robot2D::*)(const Vec&)>(&sim::Robot2D::fkine), py::arg("q"));
    // bindings.cpp:206-207: TransformedSimulationInterface(r, T)
    py::class_<sim::TransformedSimulationInterface, sim::SimulationInterface, std::shared_ptr<sim::TransformedSimulationInterface>>(m_sim, "TransformedSimulationInterface")
        .def(py::init<const std::shared_ptr<sim::SimulationInterface>&, const Mat&>(), py::arg("r"), py::arg("T"));

    // ------------------------------------------------------------------ system
    py::module m_sys = m.def_submodule("system");
    py::class_<sys::Keypoint, std::shared_ptr<sys::Keypoint>>(m_sys, "Keypoint")
        .def("diff", &sys::Keypoint::diff, py::arg("state"))
        .def("get_state", &sys::Keypoint::getState)
        .def("get_precision", &sys::Keypoint::getPrecision)
        .def("get_timestep", &sys::Keypoint::getTimestep);
    py::class_<sys::PosOrnKeypoint, sys::Keypoint, std::shared_ptr<sys::PosOrnKeypoint>>(m_sys, "PosOrnKeypoint")
        .def(py::init<const Vec&, const Vec&, const Mat&, const int&>(), py::arg("position"), py::arg("orientation"), py::arg("precision"), py::arg("timestep"))
        .def(py::init<const Vec&, const Vec&, const Vec&, const Vec&, const Mat&, const int&>(), py::arg("position"), py::arg("dposition"), py::arg("orientation"),
             py::arg("dorientation"), py::arg("precision"), py::arg("timestep"))
        .def("get_position", &sys::PosOrnKeypoint::getPosition)
        .def("get_orientation", &sys::PosOrnKeypoint::getOrientation);
    // bindings.cpp:302-306 (argument names pos_thresh / orn_thresh as there)
    py::class_<sys::PosOrnKeypointDistFunct, sys::PosOrnKeypoint, std::shared_ptr<sys::PosOrnKeypointDistFunct>>(m_sys, "PosOrnKeypointDistFunct")
        .def(py::init<const Vec&, const Vec&, const Mat&, const double&, const Vec&, const int&>(), py::arg("position"), py::arg("orientation"), py::arg("precision"),
             py::arg("pos_thresh"), py::arg("orn_thresh"), py::arg("timestep"))
        .def(py::init<const Vec&, const Vec&, const Vec&, const Vec&, const Mat&, const double&, const Vec&, const int&>(), py::arg("position"), py::arg("dposition"),
             py::arg("orientation"), py::arg("dorientation"), py::arg("precision"), py::arg("pos_thresh"), py::arg("orn_thresh"), py::arg("timestep"));
    // bindings.cpp:368-371
    py::class_<sys::AngularKeypoint, sys::Keypoint, std::shared_ptr<sys::AngularKeypoint>>(m_sys, "AngularKeypoint")
        .def(py::init<const Vec&, const Mat&, const int&>(), py::arg("position"), py::arg("precision"), py::arg("timestep"))
        .def(py::init<const Vec&, const Vec&, const Mat&, const int&>(), py::arg("position"), py::arg("dposition"), py::arg("precision"), py::arg("timestep"))
        .def("get_position", &sys::AngularKeypoint::getPosition);
    // bindings.cpp:388-392
    py::class_<sys::AngularTimeKeypoint, sys::AngularKeypoint, std::shared_ptr<sys::AngularTimeKeypoint>>(m_sys, "AngularTimeKeypoint")
        .def(py::init<const Vec&, const Mat&, const double&, const int&>(), py::arg("position"), py::arg("precision"), py::arg("continuous_time"), py::arg("timestep"))
        .def(py::init<const Vec&, const Vec&, const Mat&, const double&, const int&>(), py::arg("position"), py::arg("dposition"), py::arg("precision"),
             py::arg("continuous_time"), py::arg("timestep"))
        .def("get_continuous_time", &sys::AngularTimeKeypoint::getContinuousTime);
    py::class_<sys::SpacetimeKeypoint, sys::PosOrnKeypoint, std::shared_ptr<sys::SpacetimeKeypoint>>(m_sys, "SpacetimeKeypoint")
        .def(py::init<const Vec&, const Vec&, const Mat&, const double&, const int&>(), py::arg("position"), py::arg("orientation"), py::arg("precision"),
             py::arg("continuous_time"), py::arg("timestep"))
        .def(py::init<const Vec&, const Vec&, const Vec&, const Vec&, const Mat&, const double&, const int&>(), py::arg("position"), py::arg("dposition"),
             py::arg("orientation"), py::arg("dorientation"), py::arg("precision"), py::arg("continuous_time"), py::arg("timestep"))
        .def("get_continuous_time", &sys::SpacetimeKeypoint::getContinuousTime);
    py::class_<sys::System, std::shared_ptr<sys::System>>(m_sys, "System")
        .def("get_mu_vector", &sys::System::getMuVector, py::arg("sparse") = false)
        .def("get_Q_matrix", &sys::System::getQMatrix, py::arg("sparse") = false)
        // single-point evaluation API (bindings.cpp:414-497); host glue, the solvers run the batched device path instead
        .def("forward_pass", &sys::System::forwardPass, py::arg("xk"), py::arg("uk"), py::arg("k"))
        .def("diff", &sys::System::diff, py::arg("actual_state"), py::arg("k"))
        .def("diff_batch", &sys::System::diffBatch, py::arg("x"))
        .def("forward_pass_with_limits", &sys::System::forwardPassWithLimits, py::arg("xk"), py::arg("uk"), py::arg("k"))
        .def("forward_pass_batch", &sys::System::fpBatch, py::arg("u"))
        .def("cost_F", &sys::System::cost_F, py::arg("xk"))
        .def("cost_F_x", &sys::System::cost_F_x, py::arg("xk"))
        .def("cost_F_xx", &sys::System::cost_F_xx, py::arg("xk"))
        .def("cost", &sys::System::cost, py::arg("xk"), py::arg("uk"), py::arg("k"))
        .def("cost_x", &sys::System::cost_x, py::arg("xk"), py::arg("uk"), py::arg("k"))
        .def("cost_xx", &sys::System::cost_xx, py::arg("xk"), py::arg("uk"), py::arg("k"))
        .def("cost_u", &sys::System::cost_u, py::arg("xk"), py::arg("uk"), py::arg("k"))
        .def("cost_uu", &sys::System::cost_uu, py::arg("xk"), py::arg("uk"), py::arg("k"))
        .def("cost_xu", &sys::System::cost_xu, py::arg("xk"), py::arg("uk"), py::arg("k"))
        .def("cost_ux", &sys::System::cost_ux, py::arg("xk"), py::arg("uk"), py::arg("k"))
        .def("get_fx_jac", static_cast<std::tuple<Vec, Mat> (sys::System::*)()>(&sys::System::getFxJac))
        .def("get_fx_jac", static_cast<std::tuple<Vec, Mat> (sys::System::*)(const Vec&)>(&sys::System::getFxJac), py::arg("xk"))
        .def("get_nb_state_var", &sys::System::getNbStateVar)
        .def("get_nb_ctrl_var", &sys::System::getNbCtrlVar)
        .def("get_nb_target_var", &sys::System::getNbTargetVar)
        .def("get_horizon", &sys::System::getHorizon)
        .def("get_state", &sys::System::getState)
        .def("get_init_state", &sys::System::getInitState)
        .def("get_init_fx_state", &sys::System::getInitFoXState)
        .def("reset", &sys::System::reset);
    using KPs = std::vector<std::shared_ptr<sys::Keypoint>>;
    using SimP = std::shared_ptr<sim::SimulationInterface>;
    py::class_<sys::PosOrnPlannerSys, sys::System, std::shared_ptr<sys::PosOrnPlannerSys>>(m_sys, "PosOrnPlannerSys")
        .def(py::init<const SimP&, const KPs&, const Vec&, const Vec&, const Vec&, const Vec&, const Vec&, int, int, double>(), py::arg("r"), py::arg("keypoints"),
             py::arg("RtDiag"), py::arg("qMax"), py::arg("qMin"), py::arg("dqMax"), py::arg("dqMin"), py::arg("horizon"), py::arg("nbDeriv"), py::arg("dt"))
        .def(py::init<const SimP&, const KPs&, const Vec&, const Vec&, const Vec&, int, int, double>(), py::arg("r"), py::arg("keypoints"), py::arg("RtDiag"),
             py::arg("qMax"), py::arg("qMin"), py::arg("horizon"), py::arg("nbDeriv"), py::arg("dt"))
        .def(py::init<const SimP&, const KPs&, const Vec&, int, int, double>(), py::arg("r"), py::arg("keypoints"), py::arg("RtDiag"), py::arg("horizon"),
             py::arg("nbDeriv"), py::arg("dt"));
    // bindings.cpp:528-536
    py::class_<sys::JointSpacePlannerSys, sys::System, std::shared_ptr<sys::JointSpacePlannerSys>>(m_sys, "JointSpacePlannerSys")
        .def(py::init<const SimP&, const KPs&, const Vec&, const Vec&, const Vec&, const Vec&, const Vec&, int, int, double>(), py::arg("r"), py::arg("keypoints"),
             py::arg("RtDiag"), py::arg("qMax"), py::arg("qMin"), py::arg("dqMax"), py::arg("dqMin"), py::arg("horizon"), py::arg("nbDeriv"), py::arg("dt"))
        .def(py::init<const SimP&, const KPs&, const Vec&, const Vec&, const Vec&, int, int, double>(), py::arg("r"), py::arg("keypoints"), py::arg("RtDiag"),
             py::arg("qMax"), py::arg("qMin"), py::arg("horizon"), py::arg("nbDeriv"), py::arg("dt"))
        .def(py::init<const SimP&, const KPs&, const Vec&, int, int, double>(), py::arg("r"), py::arg("keypoints"), py::arg("RtDiag"), py::arg("horizon"), py::arg("nbDeriv"),
             py::arg("dt"));
    // bindings.cpp:571-579
    py::class_<sys::JointSpaceTimePlannerSys, sys::System, std::shared_ptr<sys::JointSpaceTimePlannerSys>>(m_sys, "JointSpaceTimePlannerSys")
        .def(py::init<const SimP&, const KPs&, const Vec&, const Vec&, const Vec&, const Vec&, const Vec&, int, int>(), py::arg("r"), py::arg("keypoints"),
             py::arg("RtDiag"), py::arg("qMax"), py::arg("qMin"), py::arg("dqMax"), py::arg("dqMin"), py::arg("horizon"), py::arg("nbDeriv"))
        .def(py::init<const SimP&, const KPs&, const Vec&, const Vec&, const Vec&, int, int>(), py::arg("r"), py::arg("keypoints"), py::arg("RtDiag"),
             py::arg("qMax"), py::arg("qMin"), py::arg("horizon"), py::arg("nbDeriv"))
        .def(py::init<const SimP&, const KPs&, const Vec&, int, int>(), py::arg("r"), py::arg("keypoints"), py::arg("RtDiag"), py::arg("horizon"), py::arg("nbDeriv"));
    py::class_<sys::PosOrnTimePlannerSys, sys::System, std::shared_ptr<sys::PosOrnTimePlannerSys>>(m_sys, "PosOrnTimePlannerSys")
        .def(py::init<const SimP&, const KPs&, const Vec&, const Vec&, const Vec&, const Vec&, const Vec&, int, int>(), py::arg("r"), py::arg("keypoints"),
             py::arg("RtDiag"), py::arg("qMax"), py::arg("qMin"), py::arg("dqMax"), py::arg("dqMin"), py::arg("horizon"), py::arg("nbDeriv"))
        .def(py::init<const SimP&, const KPs&, const Vec&, const Vec&, const Vec&, int, int>(), py::arg("r"), py::arg("keypoints"), py::arg("RtDiag"),
             py::arg("qMax"), py::arg("qMin"), py::arg("horizon"), py::arg("nbDeriv"))
        .def(py::init<const SimP&, const KPs&, const Vec&, int, int>(), py::arg("r"), py::arg("keypoints"), py::arg("RtDiag"), py::arg("horizon"), py::arg("nbDeriv"));
    // bindings.cpp:505-507: SequentialSystem(r, systems, RtDiag, horizon, nbDeriv)
    py::class_<sys::SequentialSystem, sys::System, std::shared_ptr<sys::SequentialSystem>>(m_sys, "SequentialSystem")
        .def(py::init<const SimP&, const std::vector<std::shared_ptr<sys::System>>&, const Vec&, int, int>(), py::arg("r"), py::arg("systems"), py::arg("RtDiag"),
             py::arg("horizon"), py::arg("nbDeriv"));

    // ------------------------------------------------------------------ utils (before solver: CallBackMessage is an argument type)
    py::module m_ut = m.def_submodule("utils");
    py::class_<CallBackMessage>(m_ut, "CallBackMessage");
    py::class_<PythonCallbackMessage, CallBackMessage>(m_ut, "PythonCallbackMessage").def(py::init<>());
    py::module m_sd = m_ut.def_submodule("Sd");
    m_sd.def("logMap", &Sd::logMap, py::arg("base"), py::arg("y"));
    m_sd.def("expMap", &Sd::expMap, py::arg("base"), py::arg("u"));
    m_sd.def("distance", &Sd::distance, py::arg("x"), py::arg("y"));
    m_sd.def("transport", &Sd::transport, py::arg("v"), py::arg("base1"), py::arg("base2"));
    m_sd.def("dquat_to_w_jac", &Sd::dQuatToDxJac, py::arg("q"));
    py::module m_prim = m_ut.def_submodule("primitives");
    m_prim.def("build_psi_RBF", &buildPsiRBF, py::arg("dim"), py::arg("K"));
    m_prim.def("build_psi_bernstein", &buildPsiBernstein, py::arg("dim"), py::arg("K"));
    m_prim.def("build_psi_unitstep", &buildPsiUnitstep, py::arg("dim"), py::arg("K"));
    m_prim.def("build_psi_sawtooth", &buildPsiSawtooth, py::arg("dim"), py::arg("K"));
    m_prim.def("build_psi_linear", &buildPsiLinear, py::arg("dim"), py::arg("K"));

    // ------------------------------------------------------------------ solver
    py::module m_sol = m.def_submodule("solver");
    py::class_<solver::BatchResult>(m_sol, "BatchResult")
        .def_property_readonly("X", [](const solver::BatchResult& r) { return shaped(r.X, {r.B, r.T, r.n_x}); })
        .def_property_readonly("fX", [](const solver::BatchResult& r) { return shaped(r.fX, {r.fX.empty() ? 0 : r.B, r.T, r.n_f}); })
        .def_property_readonly("U", [](const solver::BatchResult& r) { return shaped(r.U, {r.B, r.T - 1, r.n_u}); })
        .def_property_readonly("K", [](const solver::BatchResult& r) { return shaped(r.K, {r.K.empty() ? 0 : r.B, r.T - 1, r.n_u, r.n_x}); })
        .def_property_readonly("d", [](const solver::BatchResult& r) { return shaped(r.d, {r.d.empty() ? 0 : r.B, r.T - 1, r.n_u}); })
        .def_property_readonly("cost", [](const solver::BatchResult& r) { return shaped(r.cost, {r.B}); })
        .def_property_readonly("alpha", [](const solver::BatchResult& r) { return shaped(r.alpha, {r.B}); })
        .def_property_readonly("iters", [](const solver::BatchResult& r) { return py::array_t<int>(r.iters.size(), r.iters.data()); })
        .def_property_readonly("status", [](const solver::BatchResult& r) { return py::array_t<int>(r.status.size(), r.status.data()); })
        .def_property_readonly("cost_trace", [](const solver::BatchResult& r) { return shaped(r.cost_trace, {r.cost_trace.empty() ? 0 : r.B, r.nb_iter}); })
        .def_property_readonly("alpha_trace", [](const solver::BatchResult& r) { return shaped(r.alpha_trace, {r.alpha_trace.empty() ? 0 : r.B, r.nb_iter}); })
        .def_readonly("seconds", &solver::BatchResult::seconds);
    py::class_<solver::MultiStartResult, solver::BatchResult>(m_sol, "MultiStartResult")
        .def_readonly("S", &solver::MultiStartResult::S)
        .def_property_readonly("winner", [](const solver::MultiStartResult& r) { return py::array_t<int>(r.winner.size(), r.winner.data()); })
        .def_property_readonly("n_candidates", [](const solver::MultiStartResult& r) { return py::array_t<int>(r.n_candidates.size(), r.n_candidates.data()); })
        .def_property_readonly("coarse_best", [](const solver::MultiStartResult& r) { return shaped(r.coarse_best, {r.B}); })
        .def_property_readonly("coarse_first", [](const solver::MultiStartResult& r) { return shaped(r.coarse_first, {r.B}); })
        // filled when solve_multistart is given spheres, else None
        .def_property_readonly("coarse_clearance", [](const solver::MultiStartResult& r) -> py::object {
            return r.clearance.empty() ? py::object(py::none()) : py::object(shaped(r.coarse_clearance, {r.B})); })
        .def_property_readonly("clearance", [](const solver::MultiStartResult& r) -> py::object {
            return r.clearance.empty() ? py::object(py::none()) : py::object(shaped(r.clearance, {r.B})); })
        .def_property_readonly("clearance_at", [](const solver::MultiStartResult& r) -> py::object {
            if (r.clearance.empty()) return py::none();
            py::array_t<int> a({(py::ssize_t)r.B, (py::ssize_t)3});
            std::copy(r.clearance_at.begin(), r.clearance_at.end(), a.mutable_data());
            return a; })
        .def_property_readonly("n_below", [](const solver::MultiStartResult& r) -> py::object {
            return r.clearance.empty() ? py::object(py::none()) : py::object(py::array_t<int>(r.n_below.size(), r.n_below.data())); });
    py::class_<solver::ClearanceResult>(m_sol, "ClearanceResult")
        .def_property_readonly("clr", [](const solver::ClearanceResult& r) { return shaped(r.clr, {r.n, r.T}); })
        .def_property_readonly("clr_min", [](const solver::ClearanceResult& r) { return shaped(r.clr_min, {r.n}); })
        .def_property_readonly("clr_at", [](const solver::ClearanceResult& r) {
            py::array_t<int> a({(py::ssize_t)r.n, (py::ssize_t)3});
            std::copy(r.clr_at.begin(), r.clr_at.end(), a.mutable_data());
            return a; })
        .def_property_readonly("n_below", [](const solver::ClearanceResult& r) { return py::array_t<int>(r.n_below.size(), r.n_below.data()); })
        .def_property_readonly("eligible", [](const solver::ClearanceResult& r) { return py::array_t<int>(r.eligible.size(), r.eligible.data()); })
        .def_property_readonly("stats", [](const solver::ClearanceResult& r) -> py::object {
            return r.n_groups ? py::object(shaped(r.stats, {r.n_groups, ILQR_CLR_STATS})) : py::object(py::none()); });
    // clearance(system, X[n][T][n_x], spheres, ...): any trajectories in the system's state layout against sphere obstacles and planes
    m.def("clearance",
          [](const std::shared_ptr<sys::System>& s, const py::object& X, const py::object& spheres, const py::object& planes, const py::object& obstacles, double margin,
             int traj_per_set, int stats_group, const py::object& sp) {
              arr_t x = arr_t::ensure(X);
              if (!x || x.ndim() != 3) throw std::runtime_error("[clearance] X must be n x T x nb_state_var");
              if (spheres.is_none()) throw std::runtime_error("[clearance] spheres are required");
              return solver::clearance(*s, std::vector<double>(x.data(), x.data() + x.size()), (int)x.shape(0), (int)x.shape(1),
                                       clearance_inputs(spheres, planes, obstacles, margin, sp), traj_per_set, stats_group);
          },
          py::arg("system"), py::arg("X"), py::arg("spheres"), py::arg("planes") = py::none(), py::arg("obstacles") = py::none(), py::arg("margin") = 0.0,
          py::arg("traj_per_set") = 0, py::arg("stats_group") = 0, py::arg("self_pairs") = py::none());
    py::class_<solver::ClosedLoopResult>(m_sol, "ClosedLoopResult")
        .def_property_readonly("cost", [](const solver::ClosedLoopResult& r) { return shaped(r.cost, {r.B, r.S}); })
        .def_property_readonly("X", [](const solver::ClosedLoopResult& r) { return shaped(r.X, {r.B, r.S, r.T, r.n_x}); })
        .def_property_readonly("U", [](const solver::ClosedLoopResult& r) { return shaped(r.U, {r.B, r.S, r.T - 1, r.n_u}); })
        .def_property_readonly("stats", [](const solver::ClosedLoopResult& r) { return shaped(r.stats, {r.B, ILQR_CL_STATS}); })
        // filled when closed_loop_batch is given kp_tol or lim_tol, else None
        .def_property_readonly("kp_err", [](const solver::ClosedLoopResult& r) -> py::object {
            return r.outcome.empty() ? py::object(py::none()) : py::object(shaped(r.kp_err, {r.B, r.S, r.n_kp, ILQR_KP_ERR})); })
        .def_property_readonly("kp_stats", [](const solver::ClosedLoopResult& r) -> py::object {
            return r.outcome.empty() ? py::object(py::none()) : py::object(shaped(r.kp_stats, {r.B, r.n_kp, ILQR_KP_STATS})); })
        .def_property_readonly("lim_cost", [](const solver::ClosedLoopResult& r) -> py::object {
            return r.outcome.empty() ? py::object(py::none()) : py::object(shaped(r.lim_cost, {r.B, r.S})); })
        .def_property_readonly("outcome", [](const solver::ClosedLoopResult& r) -> py::object {
            return r.outcome.empty() ? py::object(py::none()) : py::object(shaped(r.outcome, {r.B, ILQR_CL_OUTCOME})); })
        // filled when AL_ILQR.closed_loop_batch is given con_tol, else None; outcome_con needs kp_tol or lim_tol as well
        .def_property_readonly("con_max", [](const solver::ClosedLoopResult& r) -> py::object {
            return r.con_stats.empty() ? py::object(py::none()) : py::object(shaped(r.con_max, {r.B, r.S})); })
        .def_property_readonly("con_steps", [](const solver::ClosedLoopResult& r) -> py::object {
            return r.con_stats.empty() ? py::object(py::none()) : py::object(shaped(r.con_steps, {r.B, r.S})); })
        .def_property_readonly("con_stats", [](const solver::ClosedLoopResult& r) -> py::object {
            return r.con_stats.empty() ? py::object(py::none()) : py::object(shaped(r.con_stats, {r.B, ILQR_CL_CON_STATS})); })
        .def_property_readonly("outcome_con", [](const solver::ClosedLoopResult& r) -> py::object {
            return r.outcome_con.empty() ? py::object(py::none()) : py::object(shaped(r.outcome_con, {r.B, ILQR_CL_OUTCOME_CON})); });
    py::class_<solver::ClosedLoopCovResult>(m_sol, "ClosedLoopCovResult")
        .def_property_readonly("Sigma", [](const solver::ClosedLoopCovResult& r) -> py::object {   // None unless want_Sigma
            return r.Sigma.empty() ? py::object(py::none()) : py::object(shaped(r.Sigma, {r.B, r.T, r.n_x, r.n_x})); })
        .def_property_readonly("kp_Sigma", [](const solver::ClosedLoopCovResult& r) { return shaped(r.kp_Sigma, {r.B, r.n_kp, r.n_x, r.n_x}); })
        .def_property_readonly("kp_var", [](const solver::ClosedLoopCovResult& r) { return shaped(r.kp_var, {r.B, r.n_kp, ILQR_CL_COV_KP}); })
        .def_property_readonly("u_var", [](const solver::ClosedLoopCovResult& r) { return shaped(r.u_var, {r.B, r.T - 1, r.n_u}); })
        .def_property_readonly("lim_z", [](const solver::ClosedLoopCovResult& r) { return shaped(r.lim_z, {r.B}); })
        // filled when AL_ILQR.closed_loop_cov_batch is given want_con, else None
        .def_property_readonly("con_var", [](const solver::ClosedLoopCovResult& r) -> py::object {
            return r.con_z.empty() ? py::object(py::none()) : py::object(shaped(r.con_var, {r.B, r.T - 1, r.m})); })
        .def_property_readonly("con_z", [](const solver::ClosedLoopCovResult& r) -> py::object {
            return r.con_z.empty() ? py::object(py::none()) : py::object(shaped(r.con_z, {r.B})); })
        // filled when closed_loop_cov_batch is given spheres (ilqr_problem_closed_loop_cov_clr), else None
        .def_property_readonly("clr_var", [](const solver::ClosedLoopCovResult& r) -> py::object {
            return r.eligible.empty() ? py::object(py::none()) : py::object(shaped(r.clr_var, {r.B, r.T})); })
        .def_property_readonly("clr_z", [](const solver::ClosedLoopCovResult& r) -> py::object {
            return r.eligible.empty() ? py::object(py::none()) : py::object(shaped(r.clr_z, {r.B, r.T})); })
        .def_property_readonly("clr_z_min", [](const solver::ClosedLoopCovResult& r) -> py::object {
            return r.eligible.empty() ? py::object(py::none()) : py::object(shaped(r.clr_z_min, {r.B})); })
        .def_property_readonly("clr_z_at", [](const solver::ClosedLoopCovResult& r) -> py::object {
            return r.eligible.empty() ? py::object(py::none()) : py::object(shaped_i(r.clr_z_at, {r.B, 3})); })
        .def_property_readonly("eligible", [](const solver::ClosedLoopCovResult& r) -> py::object {
            return r.eligible.empty() ? py::object(py::none()) : py::object(shaped_i(r.eligible, {r.B})); });
    py::class_<solver::Constraint>(m_sol, "Constraint").def(py::init<>()).def_readwrite("A", &solver::Constraint::A).def_readwrite("b", &solver::Constraint::b);
    py::class_<solver::ILQRRecursive>(m_sol, "ILQRRecursive")
        .def(py::init<const std::shared_ptr<sys::System>&>(), py::arg("s"))
        .def("solve", &solver::ILQRRecursive::solve, py::arg("U0"), py::arg("nb_iter"), py::arg("line_search"), py::arg("early_stop"), py::arg("cb"))
        .def("solve_batch",
             [](solver::ILQRRecursive& self, const py::object& U0, int nb_iter, bool ls, bool es, const py::object& q0, const py::object& dq0, const py::object& kp, bool pg,
                const py::object& spheres, const py::object& planes, const py::object& obstacles, double margin, double ow, const std::string& op, const py::object& sp) {
                 return self.solveBatch(obstacle_path(obstacle_terms(plan_gains(batch_inputs(U0, q0, dq0, kp), pg), spheres, planes, obstacles, margin, ow, sp), op, "solve_batch"), nb_iter, ls, es);
             },
             py::arg("U0"), py::arg("nb_iter"), py::arg("line_search"), py::arg("early_stop"), py::arg("q0") = py::none(), py::arg("dq0") = py::none(),
             py::arg("kp_targets") = py::none(), py::arg("plan_gains") = false, py::arg("spheres") = py::none(), py::arg("planes") = py::none(),
             py::arg("obstacles") = py::none(), py::arg("margin") = 0.0, py::arg("obstacle_weight") = 0.0, py::arg("obstacle_path") = "generic", py::arg("self_pairs") = py::none())
        // every task (the batch of U0 / q0 / kp_targets) from S starts: solve_batch's arguments, then the starts
        .def("solve_multistart",
             [](solver::ILQRRecursive& self, const py::object& U0, int nb_iter, bool ls, bool es, int S, unsigned long long seed, const py::object& sigma_u, int coarse_iter,
                const py::object& q0, const py::object& dq0, const py::object& kp, bool pg, const py::object& spheres, const py::object& planes,
                const py::object& obstacles, double margin, double ow, const std::string& op, const py::object& sp) {
                 return self.solveMultiStart(obstacle_path(plan_gains(batch_inputs(U0, q0, dq0, kp), pg), op, "solve_multistart"), multistart_inputs(S, seed, sigma_u, coarse_iter, spheres, planes, obstacles, margin, ow, sp),
                                             nb_iter, ls, es);
             },
             py::arg("U0"), py::arg("nb_iter"), py::arg("line_search"), py::arg("early_stop"), py::arg("S"), py::arg("seed") = 0, py::arg("sigma_u") = py::none(),
             py::arg("coarse_iter") = 1, py::arg("q0") = py::none(), py::arg("dq0") = py::none(), py::arg("kp_targets") = py::none(), py::arg("plan_gains") = false,
             py::arg("spheres") = py::none(), py::arg("planes") = py::none(), py::arg("obstacles") = py::none(), py::arg("margin") = 0.0, py::arg("obstacle_weight") = 0.0,
             py::arg("obstacle_path") = "generic", py::arg("self_pairs") = py::none())
        .def("closed_loop_batch",
             [](solver::ILQRRecursive& self, const py::object& U0, int nb_iter, bool ls, bool es, const py::object& q0, const py::object& dq0, const py::object& kp,
                const py::object& x0, const py::object& w, bool ff, const py::object& samples, const py::object& seed, const py::object& sigma_w,
                const py::object& sigma_x0, const py::object& kp_tol, const py::object& lim_tol, bool pg) {
                 return self.closedLoopBatch(plan_gains(batch_inputs(U0, q0, dq0, kp), pg), closed_loop_inputs(x0, w, samples, ff, seed, sigma_w, sigma_x0, kp_tol, lim_tol), nb_iter,
                                             ls, es);
             },
             py::arg("U0"), py::arg("nb_iter"), py::arg("line_search"), py::arg("early_stop"), py::arg("q0") = py::none(), py::arg("dq0") = py::none(),
             py::arg("kp_targets") = py::none(), py::arg("x0") = py::none(), py::arg("w") = py::none(), py::arg("with_feedforward") = false,
             py::arg("samples") = py::none(), py::arg("seed") = py::none(), py::arg("sigma_w") = py::none(), py::arg("sigma_x0") = py::none(), py::arg("kp_tol") = py::none(), py::arg("lim_tol") = py::none(), py::arg("plan_gains") = false)
        .def("closed_loop_cov_batch",
             [](solver::ILQRRecursive& self, const py::object& U0, int nb_iter, bool ls, bool es, const py::object& q0, const py::object& dq0, const py::object& kp,
                const py::object& sigma_w, const py::object& sigma_x0, bool want_Sigma, bool pg, const py::object& spheres, const py::object& planes, const py::object& obstacles, const py::object& self_pairs, double margin, double z_tol) {
                 return self.closedLoopCovBatch(plan_gains(batch_inputs(U0, q0, dq0, kp), pg),
                                                cov_clearance(closed_loop_cov_inputs(sigma_w, sigma_x0, want_Sigma), spheres, planes, obstacles, self_pairs, margin, z_tol), nb_iter, ls, es);
             },
             py::arg("U0"), py::arg("nb_iter"), py::arg("line_search"), py::arg("early_stop"), py::arg("q0") = py::none(), py::arg("dq0") = py::none(),
             py::arg("kp_targets") = py::none(), py::arg("sigma_w") = py::none(), py::arg("sigma_x0") = py::none(), py::arg("want_Sigma") = false, py::arg("plan_gains") = false, py::arg("spheres") = py::none(), py::arg("planes") = py::none(), py::arg("obstacles") = py::none(), py::arg("self_pairs") = py::none(), py::arg("margin") = 0.0,
             py::arg("z_tol") = 0.0);
    py::class_<solver::AL_ILQR>(m_sol, "AL_ILQR")
        .def(py::init<const std::shared_ptr<sys::System>&, const std::vector<solver::Constraint>&, const std::vector<Vec>&>(), py::arg("s"), py::arg("inequality"),
             py::arg("initLambda"))
        .def("solve", &solver::AL_ILQR::solve, py::arg("U0"), py::arg("nb_iter"), py::arg("lag_update_step"), py::arg("penalty"), py::arg("scaling_factor"),
             py::arg("line_search"), py::arg("early_stop"), py::arg("cb"))
        .def("solve_batch",
             [](solver::AL_ILQR& self, const py::object& U0, int nb_iter, int lag, double pen, double sc, bool ls, bool es, const py::object& q0, const py::object& dq0,
                const py::object& kp, bool pg, const py::object& agp, const py::object& spheres, const py::object& planes, const py::object& obstacles, double margin,
                double ow, const std::string& op, const py::object& sp) {
                 return self.solveBatch(obstacle_path(obstacle_terms(al_gains(plan_gains(batch_inputs(U0, q0, dq0, kp), pg), agp), spheres, planes, obstacles, margin, ow, sp), op, "solve_batch"), nb_iter, lag, pen,
                                        sc, ls, es);
             },
             py::arg("U0"), py::arg("nb_iter"), py::arg("lag_update_step"), py::arg("penalty"), py::arg("scaling_factor"), py::arg("line_search"),
             py::arg("early_stop"), py::arg("q0") = py::none(), py::arg("dq0") = py::none(), py::arg("kp_targets") = py::none(), py::arg("plan_gains") = false,
             py::arg("al_gains_penalty") = py::none(), py::arg("spheres") = py::none(), py::arg("planes") = py::none(), py::arg("obstacles") = py::none(),
             py::arg("margin") = 0.0, py::arg("obstacle_weight") = 0.0, py::arg("obstacle_path") = "generic", py::arg("self_pairs") = py::none())
        .def("solve_multistart",
             [](solver::AL_ILQR& self, const py::object& U0, int nb_iter, int lag, double pen, double sc, bool ls, bool es, int S, unsigned long long seed,
                const py::object& sigma_u, int coarse_iter, const py::object& q0, const py::object& dq0, const py::object& kp, bool pg, const py::object& agp,
                const py::object& spheres, const py::object& planes, const py::object& obstacles, double margin, double ow, const std::string& op, const py::object& sp) {
                 return self.solveMultiStart(obstacle_path(al_gains(plan_gains(batch_inputs(U0, q0, dq0, kp), pg), agp), op, "solve_multistart"),
                                             multistart_inputs(S, seed, sigma_u, coarse_iter, spheres, planes, obstacles, margin, ow, sp), nb_iter, lag, pen, sc, ls, es);
             },
             py::arg("U0"), py::arg("nb_iter"), py::arg("lag_update_step"), py::arg("penalty"), py::arg("scaling_factor"), py::arg("line_search"),
             py::arg("early_stop"), py::arg("S"), py::arg("seed") = 0, py::arg("sigma_u") = py::none(), py::arg("coarse_iter") = 1, py::arg("q0") = py::none(),
             py::arg("dq0") = py::none(), py::arg("kp_targets") = py::none(), py::arg("plan_gains") = false, py::arg("al_gains_penalty") = py::none(),
             py::arg("spheres") = py::none(), py::arg("planes") = py::none(), py::arg("obstacles") = py::none(), py::arg("margin") = 0.0, py::arg("obstacle_weight") = 0.0,
             py::arg("obstacle_path") = "generic", py::arg("self_pairs") = py::none())
        .def_static("final_penalty", &solver::AL_ILQR::finalPenalty, py::arg("nb_iter"), py::arg("lag_update_step"), py::arg("penalty"), py::arg("scaling_factor"))
        .def("closed_loop_batch",
             [](solver::AL_ILQR& self, const py::object& U0, int nb_iter, int lag, double pen, double sc, bool ls, bool es, const py::object& q0, const py::object& dq0,
                const py::object& kp, const py::object& x0, const py::object& w, bool ff, const py::object& samples, const py::object& seed,
                const py::object& sigma_w, const py::object& sigma_x0, const py::object& kp_tol, const py::object& lim_tol, bool pg, const py::object& con_tol,
                const py::object& agp) {
                 return self.closedLoopBatch(al_gains(plan_gains(batch_inputs(U0, q0, dq0, kp), pg), agp),
                                             closed_loop_inputs(x0, w, samples, ff, seed, sigma_w, sigma_x0, kp_tol, lim_tol, con_tol), nb_iter, lag, pen, sc, ls, es);
             },
             py::arg("U0"), py::arg("nb_iter"), py::arg("lag_update_step"), py::arg("penalty"), py::arg("scaling_factor"), py::arg("line_search"),
             py::arg("early_stop"), py::arg("q0") = py::none(), py::arg("dq0") = py::none(), py::arg("kp_targets") = py::none(), py::arg("x0") = py::none(),
             py::arg("w") = py::none(), py::arg("with_feedforward") = false, py::arg("samples") = py::none(), py::arg("seed") = py::none(),
             py::arg("sigma_w") = py::none(), py::arg("sigma_x0") = py::none(), py::arg("kp_tol") = py::none(), py::arg("lim_tol") = py::none(), py::arg("plan_gains") = false,
             py::arg("con_tol") = py::none(), py::arg("al_gains_penalty") = py::none())
        .def("closed_loop_cov_batch",
             [](solver::AL_ILQR& self, const py::object& U0, int nb_iter, int lag, double pen, double sc, bool ls, bool es, const py::object& q0, const py::object& dq0,
                const py::object& kp, const py::object& sigma_w, const py::object& sigma_x0, bool want_Sigma, bool pg, bool want_con,
                const py::object& agp, const py::object& spheres, const py::object& planes, const py::object& obstacles, const py::object& self_pairs, double margin, double z_tol) {
                 return self.closedLoopCovBatch(al_gains(plan_gains(batch_inputs(U0, q0, dq0, kp), pg), agp),
                                                cov_clearance(closed_loop_cov_inputs(sigma_w, sigma_x0, want_Sigma, want_con), spheres, planes, obstacles, self_pairs, margin, z_tol), nb_iter, lag,
                                                pen, sc, ls, es);
             },
             py::arg("U0"), py::arg("nb_iter"), py::arg("lag_update_step"), py::arg("penalty"), py::arg("scaling_factor"), py::arg("line_search"),
             py::arg("early_stop"), py::arg("q0") = py::none(), py::arg("dq0") = py::none(), py::arg("kp_targets") = py::none(),
             py::arg("sigma_w") = py::none(), py::arg("sigma_x0") = py::none(), py::arg("want_Sigma") = false, py::arg("plan_gains") = false,
             py::arg("want_con") = false, py::arg("al_gains_penalty") = py::none(), py::arg("spheres") = py::none(), py::arg("planes") = py::none(), py::arg("obstacles") = py::none(), py::arg("self_pairs") = py::none(), py::arg("margin") = 0.0,
             py::arg("z_tol") = 0.0);
    // bindings.cpp:778-782
    py::class_<solver::BatchILQR>(m_sol, "BatchILQR")
        .def(py::init<const std::shared_ptr<sys::System>&, const Mat&>(), py::arg("s"), py::arg("Q"))
        .def(py::init<const std::shared_ptr<sys::System>&>(), py::arg("s"))
        .def("solve", &solver::BatchILQR::solve, py::arg("nb_iter"), py::arg("u0"), py::arg("early_stop"), py::arg("cb"))
        .def("solve_batch",
             [](solver::BatchILQR& self, int nb_iter, const py::object& u0, bool es, const py::object& q0, const py::object& dq0, const py::object& kp, bool pg) {
                 return self.solveBatch(plan_gains(batch_inputs(u0, q0, dq0, kp, true), pg), nb_iter, es);
             },
             py::arg("nb_iter"), py::arg("u0"), py::arg("early_stop"), py::arg("q0") = py::none(), py::arg("dq0") = py::none(), py::arg("kp_targets") = py::none(), py::arg("plan_gains") = false)
        // the arguments of solve_batch, then the closed-loop arguments of ILQRRecursive's methods; always on the gains about the solve's plan
        .def("closed_loop_batch",
             [](solver::BatchILQR& self, int nb_iter, const py::object& u0, bool es, const py::object& q0, const py::object& dq0, const py::object& kp,
                const py::object& x0, const py::object& w, bool ff, const py::object& samples, const py::object& seed, const py::object& sigma_w,
                const py::object& sigma_x0, const py::object& kp_tol, const py::object& lim_tol) {
                 return self.closedLoopBatch(batch_inputs(u0, q0, dq0, kp, true), closed_loop_inputs(x0, w, samples, ff, seed, sigma_w, sigma_x0, kp_tol, lim_tol),
                                             nb_iter, es);
             },
             py::arg("nb_iter"), py::arg("u0"), py::arg("early_stop"), py::arg("q0") = py::none(), py::arg("dq0") = py::none(), py::arg("kp_targets") = py::none(),
             py::arg("x0") = py::none(), py::arg("w") = py::none(), py::arg("with_feedforward") = false, py::arg("samples") = py::none(),
             py::arg("seed") = py::none(), py::arg("sigma_w") = py::none(), py::arg("sigma_x0") = py::none(), py::arg("kp_tol") = py::none(),
             py::arg("lim_tol") = py::none())
        .def("closed_loop_cov_batch",
             [](solver::BatchILQR& self, int nb_iter, const py::object& u0, bool es, const py::object& q0, const py::object& dq0, const py::object& kp,
                const py::object& sigma_w, const py::object& sigma_x0, bool want_Sigma, const py::object& spheres, const py::object& planes, const py::object& obstacles, const py::object& self_pairs, double margin, double z_tol) {
                 return self.closedLoopCovBatch(batch_inputs(u0, q0, dq0, kp, true),
                                                cov_clearance(closed_loop_cov_inputs(sigma_w, sigma_x0, want_Sigma), spheres, planes, obstacles, self_pairs, margin, z_tol), nb_iter, es);
             },
             py::arg("nb_iter"), py::arg("u0"), py::arg("early_stop"), py::arg("q0") = py::none(), py::arg("dq0") = py::none(), py::arg("kp_targets") = py::none(),
             py::arg("sigma_w") = py::none(), py::arg("sigma_x0") = py::none(), py::arg("want_Sigma") = false, py::arg("spheres") = py::none(), py::arg("planes") = py::none(), py::arg("obstacles") = py::none(), py::arg("self_pairs") = py::none(), py::arg("margin") = 0.0,
             py::arg("z_tol") = 0.0);
    // bindings.cpp:862-869: positional arguments only, no defaults
    py::class_<solver::LQT>(m_sol, "LQT")
        .def(py::init<const Mat&, const Mat&, const std::vector<Mat>&, const Vec&, float, int>())
        .def("solve_DP", &solver::LQT::solveDP)
        .def("solve_lin_al", &solver::LQT::solveLinAl)
        .def("get_nb_states", &solver::LQT::getNbStates)
        .def("get_predicted_states", &solver::LQT::getPredictedStates)
        .def("get_command", static_cast<Vec (solver::LQT::*)(int)>(&solver::LQT::getCommand))
        .def("get_command", static_cast<Vec (solver::LQT::*)(int, const Vec&)>(&solver::LQT::getCommand));
    py::class_<solver::BatchILQRCP>(m_sol, "BatchILQRCP")
        .def(py::init<const std::shared_ptr<sys::System>&, const Mat&, const Mat&>(), py::arg("s"), py::arg("Q"), py::arg("psi"))
        .def(py::init<const std::shared_ptr<sys::System>&, const Mat&>(), py::arg("s"), py::arg("psi"))
        .def("solve", &solver::BatchILQRCP::solve, py::arg("nb_iter"), py::arg("u0"), py::arg("early_stop"), py::arg("cb"))
        .def("solve_batch",
             [](solver::BatchILQRCP& self, int nb_iter, const py::object& u0, bool es, const py::object& q0, const py::object& dq0, const py::object& kp, bool pg) {
                 return self.solveBatch(plan_gains(batch_inputs(u0, q0, dq0, kp, true), pg), nb_iter, es);
             },
             py::arg("nb_iter"), py::arg("u0"), py::arg("early_stop"), py::arg("q0") = py::none(), py::arg("dq0") = py::none(), py::arg("kp_targets") = py::none(), py::arg("plan_gains") = false)
        // the arguments of solve_batch, then the closed-loop arguments of ILQRRecursive's methods; always on the gains about the solve's plan
        .def("closed_loop_batch",
             [](solver::BatchILQRCP& self, int nb_iter, const py::object& u0, bool es, const py::object& q0, const py::object& dq0, const py::object& kp,
                const py::object& x0, const py::object& w, bool ff, const py::object& samples, const py::object& seed, const py::object& sigma_w,
                const py::object& sigma_x0, const py::object& kp_tol, const py::object& lim_tol) {
                 return self.closedLoopBatch(batch_inputs(u0, q0, dq0, kp, true), closed_loop_inputs(x0, w, samples, ff, seed, sigma_w, sigma_x0, kp_tol, lim_tol),
                                             nb_iter, es);
             },
             py::arg("nb_iter"), py::arg("u0"), py::arg("early_stop"), py::arg("q0") = py::none(), py::arg("dq0") = py::none(), py::arg("kp_targets") = py::none(),
             py::arg("x0") = py::none(), py::arg("w") = py::none(), py::arg("with_feedforward") = false, py::arg("samples") = py::none(),
             py::arg("seed") = py::none(), py::arg("sigma_w") = py::none(), py::arg("sigma_x0") = py::none(), py::arg("kp_tol") = py::none(),
             py::arg("lim_tol") = py::none())
        .def("closed_loop_cov_batch",
             [](solver::BatchILQRCP& self, int nb_iter, const py::object& u0, bool es, const py::object& q0, const py::object& dq0, const py::object& kp,
                const py::object& sigma_w, const py::object& sigma_x0, bool want_Sigma, const py::object& spheres, const py::object& planes, const py::object& obstacles, const py::object& self_pairs, double margin, double z_tol) {
                 return self.closedLoopCovBatch(batch_inputs(u0, q0, dq0, kp, true),
                                                cov_clearance(closed_loop_cov_inputs(sigma_w, sigma_x0, want_Sigma), spheres, planes, obstacles, self_pairs, margin, z_tol), nb_iter, es);
             },
             py::arg("nb_iter"), py::arg("u0"), py::arg("early_stop"), py::arg("q0") = py::none(), py::arg("dq0") = py::none(), py::arg("kp_targets") = py::none(),
             py::arg("sigma_w") = py::none(), py::arg("sigma_x0") = py::none(), py::arg("want_Sigma") = false, py::arg("spheres") = py::none(), py::arg("planes") = py::none(), py::arg("obstacles") = py::none(), py::arg("self_pairs") = py::none(), py::arg("margin") = 0.0,
             py::arg("z_tol") = 0.0);
}
