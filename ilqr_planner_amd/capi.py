"""ctypes binding of the C ABI in include/ilqr_hip.h (libilqr_hip.so, hand-written HIP for gfx950).

This is plumbing: every computation happens inside the shared library on the GPU.  There is no CPU fallback --
if the library is missing or no HIP device is visible, construction raises.
"""
from __future__ import annotations

import collections
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libilqr_hip.so")

MAX_SEG, MAX_KP, MAX_NX, MAX_NU, MAX_NF, MAX_NQ = 24, 8, 15, 8, 15, 13
SYS_POS_ORN, SYS_POS_ORN_TIME, SYS_JOINT, SYS_JOINT_TIME = 0, 1, 2, 3
STATUS_OK, STATUS_NONFINITE, STATUS_ALPHA_FLOOR, STATUS_SWEEP_IO = 0, 1, 2, 4  # ILQR_STATUS_* (bits of the per-instance status word)
LQT_MAX_NX, LQT_MAX_NU = 16, 8
CL_STATS = 5  # mean, variance, min, max, n_bad (ILQR_CL_STATS)
KP_ERR, KP_STATS, CL_OUTCOME = 5, 12, 4  # ILQR_KP_ERR (pos, orn, vel, angvel, time), ILQR_KP_STATS (mean[5], max[5], n_miss, n_bad), ILQR_CL_OUTCOME
CL_CON_STATS, CL_OUTCOME_CON = 6, 5  # ILQR_CL_CON_STATS (mean/max con_max, mean/max con_steps, n_con, n_bad), ILQR_CL_OUTCOME_CON (n_ok, n_miss, n_lim, n_con, n_bad)
KP_ERR_POS, KP_ERR_ORN, KP_ERR_VEL, KP_ERR_ANGVEL, KP_ERR_TIME = range(5)
PROF_ROLLOUT, PROF_BACKWARD, PROF_FORWARD, PROF_OTHER, PROF_APPLY = 0, 1, 2, 3, 4
ADOPT_STATE, ADOPT_TARGETS, ADOPT_CONTROLS0, ADOPT_CONTROLS, ADOPT_MULTIPLIERS = 1, 2, 4, 8, 16  # ILQR_ADOPT_* (bits of ilqr_problem_adopt's `what`)
CLR_MAX_SPH, CLR_MAX_PLANES, CLR_STATS = 32, 8, 4  # ILQR_CLR_MAX_SPH, ILQR_CLR_MAX_PLANES, ILQR_CLR_STATS (mean, min, n_hit, n_bad)
CLR_MAX_SELF, CLR_MAX_ANCHOR = 64, 8  # ILQR_CLR_MAX_SELF, ILQR_CLR_MAX_ANCHOR

# every symbol include/ilqr_hip.h declares (checked by tests/test_capi_symbols.py)
EXPORTS = [
    "ilqr_dims_of", "ilqr_desc_defaults", "ilqr_ctx_create", "ilqr_ctx_destroy", "ilqr_last_error", "ilqr_ctx_set_stream",
    "ilqr_ctx_synchronize", "ilqr_version", "ilqr_problem_create", "ilqr_problem_destroy", "ilqr_problem_set_init_state",
    "ilqr_problem_set_keypoint_targets", "ilqr_problem_set_controls", "ilqr_problem_set_constraints",
    "ilqr_problem_set_init_state_dev", "ilqr_problem_set_keypoint_targets_dev", "ilqr_problem_set_controls_dev",
    "ilqr_solve_recursive", "ilqr_solve_al", "ilqr_solve_batch_cp", "ilqr_solve_batch", "ilqr_problem_get_X", "ilqr_problem_get_fX",
    "ilqr_problem_get_U", "ilqr_problem_get_K", "ilqr_problem_get_d", "ilqr_problem_get_cost", "ilqr_problem_get_alpha",
    "ilqr_problem_get_iters", "ilqr_problem_get_status", "ilqr_problem_get_lambda", "ilqr_problem_get_trace",
    "ilqr_problem_get_X_dev", "ilqr_problem_get_U_dev", "ilqr_problem_get_cost_dev", "ilqr_fk_batch",
    "ilqr_profile_enable", "ilqr_profile_reset", "ilqr_profile_get", "ilqr_chain_from_urdf", "ilqr_urdf_last_error",
    "ilqr_problem_reset_multipliers", "ilqr_problem_warm_start", "ilqr_problem_track", "ilqr_problem_track_dev",
    "ilqr_problem_closed_loop", "ilqr_problem_closed_loop_dev", "ilqr_problem_closed_loop_noise", "ilqr_problem_closed_loop_noise_dev",
    "ilqr_problem_closed_loop_report", "ilqr_problem_closed_loop_report_dev", "ilqr_problem_closed_loop_cov", "ilqr_problem_closed_loop_cov_dev",
    "ilqr_problem_closed_loop_report_con", "ilqr_problem_closed_loop_report_con_dev", "ilqr_problem_closed_loop_cov_con",
    "ilqr_problem_closed_loop_cov_con_dev", "ilqr_problem_closed_loop_cov_clr", "ilqr_problem_closed_loop_cov_clr_dev",
    "ilqr_ctx_set_split", "ilqr_ctx_set_crosscheck", "ilqr_problem_gains", "ilqr_problem_gains_al",
    "ilqr_problem_adopt", "ilqr_problem_adopt_dev", "ilqr_problem_spread_controls", "ilqr_problem_spread_controls_dev",
    "ilqr_problem_select", "ilqr_problem_select_dev", "ilqr_problem_get_at", "ilqr_problem_get_at_dev",
    "ilqr_problem_clearance", "ilqr_problem_clearance_dev", "ilqr_clearance_trajectories", "ilqr_clearance_trajectories_dev",
    "ilqr_problem_set_obstacles", "ilqr_problem_set_obstacles_dev", "ilqr_problem_obstacle_terms", "ilqr_problem_obstacle_terms_dev",
    "ilqr_ctx_set_obstacle_path",
    "ilqr_lqt_create", "ilqr_lqt_destroy", "ilqr_lqt_set_targets", "ilqr_lqt_set_targets_dev", "ilqr_lqt_solve_dp", "ilqr_lqt_solve_lin_al",
    "ilqr_lqt_command", "ilqr_lqt_command_dev", "ilqr_lqt_get_U", "ilqr_lqt_get_U_dev", "ilqr_lqt_get_X", "ilqr_lqt_get_X_dev", "ilqr_lqt_get_P",
    "ilqr_lqt_get_d",
]


class ProblemDesc(C.Structure):
    """Mirror of ilqr_problem_desc."""

    _fields_ = [
        ("kind", C.c_int),
        ("nb_deriv", C.c_int),
        ("dof", C.c_int),
        ("horizon", C.c_int),
        ("dt", C.c_double),
        ("R_diag", C.c_double * MAX_NU),
        ("limits_set", C.c_int),
        ("penalty", C.c_double),
        ("state_max", C.c_double * (MAX_NX + 1)),
        ("state_min", C.c_double * (MAX_NX + 1)),
        ("limit_weight", C.c_int * (MAX_NX + 1)),
        ("n_seg", C.c_int),
        ("seg_joint", C.c_int * MAX_SEG),
        ("seg_xyz", (C.c_double * 3) * MAX_SEG),
        ("seg_R", (C.c_double * 9) * MAX_SEG),
        ("seg_axis", (C.c_double * 3) * MAX_SEG),
        ("n_kp", C.c_int),
        ("kp_timestep", C.c_int * MAX_KP),
        ("kp_Q", (C.c_double * (MAX_NQ * MAX_NQ)) * MAX_KP),
        ("kp_dist", C.c_int * MAX_KP),
        ("kp_pos_radius", C.c_double * MAX_KP),
        ("kp_orn_thresh", (C.c_double * 3) * MAX_KP),
        ("kp_has_frame", C.c_int * MAX_KP),
        ("kp_frame_R", (C.c_double * 9) * MAX_KP),
        ("kp_frame_p", (C.c_double * 3) * MAX_KP),
        ("kp_has_Ru", C.c_int * MAX_KP),
        ("kp_Ru", (C.c_double * MAX_NU) * MAX_KP),
        ("kp_joint", C.c_int * MAX_KP),
        ("limit_multiplicity", C.c_int),
        ("is_sequence", C.c_int),
        ("limits2_set", C.c_int),
        ("penalty2", C.c_double),
        ("state_max2", C.c_double * (MAX_NX + 1)),
        ("state_min2", C.c_double * (MAX_NX + 1)),
        ("limit_weight2", C.c_int * (MAX_NX + 1)),
        ("limit_multiplicity2", C.c_int),
        ("reg", C.c_double),
        ("alpha_floor", C.c_double),
        ("stop_tol", C.c_double),
    ]


class Dims(C.Structure):
    _fields_ = [("n_x", C.c_int), ("n_u", C.c_int), ("n_f", C.c_int), ("n_Q", C.c_int)]


class Noise(C.Structure):
    """Mirror of ilqr_noise."""

    _fields_ = [("seed", C.c_ulonglong), ("instance_offset", C.c_uint), ("sample_offset", C.c_uint), ("sigma_w", C.c_double * MAX_NX),
                ("sigma_x0", C.c_double * MAX_NX)]


class Seeds(C.Structure):
    """Mirror of ilqr_seeds."""

    _fields_ = [("seed", C.c_ulonglong), ("group_offset", C.c_uint), ("member_offset", C.c_uint), ("sigma_u", C.c_double * MAX_NU)]


class Tol(C.Structure):
    """Mirror of ilqr_cl_tol."""

    _fields_ = [("kp_tol", (C.c_double * KP_ERR) * MAX_KP), ("lim_tol", C.c_double)]


class Report(C.Structure):
    """Mirror of ilqr_cl_report: four pointers (host or device), 0 / None where the output is not asked for."""

    _fields_ = [("kp_err", C.c_void_p), ("kp_stats", C.c_void_p), ("lim_cost", C.c_void_p), ("outcome", C.c_void_p)]


class Cov(C.Structure):
    """Mirror of ilqr_cl_cov: five pointers (host or device), 0 / None where the output is not asked for."""

    _fields_ = [("Sigma", C.c_void_p), ("kp_Sigma", C.c_void_p), ("kp_var", C.c_void_p), ("u_var", C.c_void_p), ("lim_z", C.c_void_p)]


class Con(C.Structure):
    """Mirror of ilqr_cl_con: four pointers (host or device), 0 / None where the output is not asked for."""

    _fields_ = [("con_max", C.c_void_p), ("con_steps", C.c_void_p), ("con_stats", C.c_void_p), ("outcome_con", C.c_void_p)]


class CovCon(C.Structure):
    """Mirror of ilqr_cl_cov_con: two pointers (host or device), 0 / None where the output is not asked for."""

    _fields_ = [("con_var", C.c_void_p), ("con_z", C.c_void_p)]


class ClCovClr(C.Structure):
    """Mirror of ilqr_cl_cov_clr: five pointers (host or device), 0 / None where the output is not asked for."""

    _fields_ = [("clr_var", C.c_void_p), ("clr_z", C.c_void_p), ("clr_z_min", C.c_void_p), ("clr_z_at", C.c_void_p), ("eligible", C.c_void_p)]


class ClrRobot(C.Structure):
    """Mirror of ilqr_clr_robot."""

    _fields_ = [("n_sph", C.c_int), ("sph_link", C.c_int * CLR_MAX_SPH), ("sph_c", (C.c_double * 3) * CLR_MAX_SPH), ("sph_r", C.c_double * CLR_MAX_SPH),
                ("n_planes", C.c_int), ("plane_n", (C.c_double * 3) * CLR_MAX_PLANES), ("plane_d", C.c_double * CLR_MAX_PLANES),
                ("n_self", C.c_int), ("self_pair", (C.c_int * 2) * CLR_MAX_SELF)]


class ClrWorld(C.Structure):
    """Mirror of ilqr_clr_world: obs is a host or device pointer."""

    _fields_ = [("obs", C.c_void_p), ("n_sets", C.c_int), ("n_obs", C.c_int), ("traj_per_set", C.c_int), ("margin", C.c_double), ("stats_group", C.c_int)]


class ClrOut(C.Structure):
    """Mirror of ilqr_clr_out: six pointers (host or device), 0 / None where the output is not asked for."""

    _fields_ = [("clr", C.c_void_p), ("clr_min", C.c_void_p), ("clr_at", C.c_void_p), ("n_below", C.c_void_p), ("eligible", C.c_void_p), ("stats", C.c_void_p)]


def clr_robot(spheres, planes=None, self_pairs=None):
    """ClrRobot from spheres = [(link, (cx, cy, cz), r), ...] in chain order, planes = [((nx, ny, nz), d), ...] (n . p >= d) and
    self_pairs = [(a, b), ...]: sphere indices with a < b on different links (the robot against itself)."""
    rb = ClrRobot()
    spheres, planes, self_pairs = list(spheres), list(planes or []), list(self_pairs if self_pairs is not None else [])
    if len(spheres) > CLR_MAX_SPH or len(planes) > CLR_MAX_PLANES or len(self_pairs) > CLR_MAX_SELF:
        raise ValueError(f"at most {CLR_MAX_SPH} spheres, {CLR_MAX_PLANES} planes and {CLR_MAX_SELF} self pairs")
    rb.n_self = len(self_pairs)
    for e, (a, b) in enumerate(self_pairs):
        rb.self_pair[e][0], rb.self_pair[e][1] = int(a), int(b)
    rb.n_sph, rb.n_planes = len(spheres), len(planes)
    for i, (link, c, r) in enumerate(spheres):
        rb.sph_link[i], rb.sph_r[i] = int(link), float(r)
        for a in range(3):
            rb.sph_c[i][a] = float(c[a])
    for l, (nn, d) in enumerate(planes):
        rb.plane_d[l] = float(d)
        for a in range(3):
            rb.plane_n[l][a] = float(nn[a])
    return rb


def _clr_host_call(fn, n, T, robot, obstacles, traj_per_set, margin, stats_group, want):
    """The host form of a clearance call: fn(robot*, world*, out*) -> rc.  obstacles [n_sets][n_obs][4] or None; returns a Clearance."""
    tps = int(traj_per_set)
    obs = _f64(obstacles) if obstacles is not None else np.zeros((n // tps if tps >= 1 else 0, 0, 4))   # planes only: empty sets
    if obs.ndim != 3 or obs.shape[2] != 4:
        raise ValueError(f"obstacles: expected [n_sets][n_obs][4], got {obs.shape}")
    w = ClrWorld(obs.ctypes.data if obs.size else None, obs.shape[0], obs.shape[1], tps, float(margin), int(stats_group or 0))
    ng = n // int(stats_group) if stats_group and int(stats_group) >= 1 else 0
    clr, cmin = _out("clr" in want, n, T), _out("clr_min" in want, n)
    at = np.empty((n, 3), dtype=np.int32) if "clr_at" in want else None
    nb = np.empty(n, dtype=np.int32) if "n_below" in want else None
    el = np.empty(n, dtype=np.int32) if "eligible" in want else None
    st = _out("stats" in want, ng, CLR_STATS)
    o = ClrOut(*(a.ctypes.data if a is not None else None for a in (clr, cmin, at, nb, el, st)))
    fn(C.byref(robot), C.byref(w), C.byref(o))
    return Clearance(clr, cmin, at, nb, el, st)


CLR_OUTPUTS = ("clr", "clr_min", "clr_at", "n_below", "eligible")
Clearance = collections.namedtuple("Clearance", "clr clr_min clr_at n_below eligible stats")
ClosedLoopCov = collections.namedtuple("ClosedLoopCov", "Sigma kp_Sigma kp_var u_var lim_z")
ClosedLoopReportCon = collections.namedtuple("ClosedLoopReportCon", "cost stats kp_err kp_stats lim_cost outcome con_max con_steps con_stats outcome_con")
ClosedLoopCovCon = collections.namedtuple("ClosedLoopCovCon", "Sigma kp_Sigma kp_var u_var lim_z con_var con_z")
COV_CLR_OUTPUTS = ("clr_var", "clr_z", "clr_z_min", "clr_z_at", "eligible")
ClosedLoopCovClr = collections.namedtuple("ClosedLoopCovClr", "Sigma kp_Sigma kp_var u_var lim_z clr_var clr_z clr_z_min clr_z_at eligible")
ClosedLoopNoise = collections.namedtuple("ClosedLoopNoise", "cost stats X U w")
ClosedLoopReport = collections.namedtuple("ClosedLoopReport", "cost stats kp_err kp_stats lim_cost outcome X U w")
Selection = collections.namedtuple("Selection", "winner best n_candidates")
ObstacleTerms = collections.namedtuple("ObstacleTerms", "cost lx lxx")
Rows = collections.namedtuple("Rows", "X U cost iters status")

_lib = None


def load():
    """dlopen libilqr_hip.so and declare the prototypes.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    L.ilqr_version.restype = C.c_char_p
    L.ilqr_last_error.restype = C.c_char_p
    L.ilqr_last_error.argtypes = [vp]
    L.ilqr_desc_defaults.argtypes = [C.POINTER(ProblemDesc)]
    L.ilqr_desc_defaults.restype = None
    L.ilqr_dims_of.argtypes = [C.POINTER(ProblemDesc), C.POINTER(Dims)]
    L.ilqr_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.ilqr_ctx_destroy.argtypes = [vp]
    L.ilqr_ctx_destroy.restype = None
    L.ilqr_ctx_set_stream.argtypes = [vp, vp]
    L.ilqr_ctx_synchronize.argtypes = [vp]
    L.ilqr_ctx_set_split.argtypes = [vp, C.c_int]
    L.ilqr_ctx_set_obstacle_path.argtypes = [vp, C.c_int]
    L.ilqr_ctx_set_crosscheck.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.ilqr_problem_create.argtypes = [vp, C.POINTER(ProblemDesc), C.c_int, C.POINTER(vp)]
    L.ilqr_problem_destroy.argtypes = [vp]
    L.ilqr_problem_destroy.restype = None
    for n in ("ilqr_problem_set_init_state", "ilqr_problem_set_init_state_dev"):
        getattr(L, n).argtypes = [vp, vp, vp]
    for n in ("ilqr_problem_set_keypoint_targets", "ilqr_problem_set_keypoint_targets_dev"):
        getattr(L, n).argtypes = [vp, C.c_int, vp]
    for n in ("ilqr_problem_set_controls", "ilqr_problem_set_controls_dev"):
        getattr(L, n).argtypes = [vp, vp]
    L.ilqr_problem_set_constraints.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp]
    L.ilqr_problem_reset_multipliers.argtypes = [vp]
    L.ilqr_problem_warm_start.argtypes = [vp, C.c_int]
    L.ilqr_problem_gains.argtypes = [vp]
    L.ilqr_problem_gains_al.argtypes = [vp, C.c_double]
    for n in ("ilqr_problem_adopt", "ilqr_problem_adopt_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, C.c_int]
    for n in ("ilqr_problem_spread_controls", "ilqr_problem_spread_controls_dev"):
        getattr(L, n).argtypes = [vp, C.c_int, C.POINTER(Seeds)]
    for n in ("ilqr_problem_select", "ilqr_problem_select_dev"):
        getattr(L, n).argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    for n in ("ilqr_problem_get_at", "ilqr_problem_get_at_dev"):
        getattr(L, n).argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
    for n in ("ilqr_problem_clearance", "ilqr_problem_clearance_dev"):
        getattr(L, n).argtypes = [vp, C.POINTER(ClrRobot), C.POINTER(ClrWorld), C.POINTER(ClrOut)]
    for n in ("ilqr_clearance_trajectories", "ilqr_clearance_trajectories_dev"):
        getattr(L, n).argtypes = [vp, C.POINTER(ProblemDesc), C.c_int, C.c_int, vp, C.POINTER(ClrRobot), C.POINTER(ClrWorld), C.POINTER(ClrOut)]
    for n in ("ilqr_problem_set_obstacles", "ilqr_problem_set_obstacles_dev"):
        getattr(L, n).argtypes = [vp, C.POINTER(ClrRobot), C.POINTER(ClrWorld), C.c_double]
    for n in ("ilqr_problem_obstacle_terms", "ilqr_problem_obstacle_terms_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp]
    L.ilqr_problem_track.argtypes = [vp, C.c_int, dp, C.c_int, dp]
    L.ilqr_problem_track_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp]
    L.ilqr_problem_closed_loop.argtypes = [vp, C.c_int, dp, dp, C.c_int, dp, dp, dp]
    L.ilqr_problem_closed_loop_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp]
    L.ilqr_problem_closed_loop_noise.argtypes = [vp, C.c_int, C.POINTER(Noise), dp, C.c_int, dp, dp, dp, dp, dp]
    L.ilqr_problem_closed_loop_noise_dev.argtypes = [vp, C.c_int, C.POINTER(Noise), vp, C.c_int, vp, vp, vp, vp, vp]
    L.ilqr_problem_closed_loop_report.argtypes = [vp, C.c_int, C.POINTER(Noise), dp, dp, C.c_int, C.POINTER(Tol), dp, dp, C.POINTER(Report)]
    L.ilqr_problem_closed_loop_report_dev.argtypes = [vp, C.c_int, C.POINTER(Noise), vp, vp, C.c_int, C.POINTER(Tol), vp, vp, C.POINTER(Report)]
    L.ilqr_problem_closed_loop_cov.argtypes = [vp, dp, dp, C.POINTER(Cov)]
    L.ilqr_problem_closed_loop_cov_dev.argtypes = [vp, dp, dp, C.POINTER(Cov)]
    L.ilqr_problem_closed_loop_report_con.argtypes = [vp, C.c_int, C.POINTER(Noise), dp, dp, C.c_int, C.POINTER(Tol), dp, dp, C.POINTER(Report),
                                                      C.c_double, C.POINTER(Con)]
    L.ilqr_problem_closed_loop_report_con_dev.argtypes = [vp, C.c_int, C.POINTER(Noise), vp, vp, C.c_int, C.POINTER(Tol), vp, vp, C.POINTER(Report),
                                                          C.c_double, C.POINTER(Con)]
    L.ilqr_problem_closed_loop_cov_con.argtypes = [vp, dp, dp, C.POINTER(Cov), C.POINTER(CovCon)]
    L.ilqr_problem_closed_loop_cov_con_dev.argtypes = [vp, dp, dp, C.POINTER(Cov), C.POINTER(CovCon)]
    for n in ("ilqr_problem_closed_loop_cov_clr", "ilqr_problem_closed_loop_cov_clr_dev"):
        getattr(L, n).argtypes = [vp, dp, dp, C.POINTER(Cov), C.POINTER(ClrRobot), C.POINTER(ClrWorld), C.c_double, C.POINTER(ClCovClr)]
    L.ilqr_solve_recursive.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.ilqr_solve_al.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]
    L.ilqr_solve_batch_cp.argtypes = [vp, dp, C.c_int, C.c_int, C.c_int]
    L.ilqr_solve_batch.argtypes = [vp, C.c_int, C.c_int]
    for n in ("X", "fX", "U", "K", "d", "cost", "alpha", "lambda", "X_dev", "U_dev", "cost_dev"):
        getattr(L, "ilqr_problem_get_" + n).argtypes = [vp, vp]
    L.ilqr_problem_get_iters.argtypes = [vp, ip]
    L.ilqr_problem_get_status.argtypes = [vp, ip]
    L.ilqr_problem_get_trace.argtypes = [vp, dp, dp, C.c_int]
    L.ilqr_fk_batch.argtypes = [vp, C.POINTER(ProblemDesc), C.c_int, dp, dp, dp, dp]
    L.ilqr_profile_enable.argtypes = [vp, C.c_int]
    L.ilqr_profile_reset.argtypes = [vp]
    L.ilqr_profile_get.argtypes = [vp, C.c_int, dp, ip]
    L.ilqr_chain_from_urdf.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, dp, dp, C.POINTER(ProblemDesc), dp, dp]
    L.ilqr_urdf_last_error.restype = C.c_char_p
    _lib = L
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _f64(x, shape=None):
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
    return a


def _out(want, *shape):
    """An output array of a call, or None where it is not asked for."""
    return np.empty(shape) if want else None


def chain_from_urdf(urdf_text: str, base: str, tip: str, tool_rpy=None, tool_xyz=None):
    """URDF text -> chain dict (seg_joint, seg_xyz, seg_R, seg_axis, dof, lower, upper) via the C++ reader in the library."""
    L = load()
    d = ProblemDesc()
    L.ilqr_desc_defaults(C.byref(d))
    lo, up = np.zeros(MAX_SEG), np.zeros(MAX_SEG)
    rpy = _f64(tool_rpy, (3,)) if tool_rpy is not None else None
    xyz = _f64(tool_xyz, (3,)) if tool_xyz is not None else None
    if L.ilqr_chain_from_urdf(urdf_text.encode(), base.encode(), tip.encode(), _dp(rpy), _dp(xyz), C.byref(d), _dp(lo), _dp(up)):
        raise RuntimeError(L.ilqr_urdf_last_error().decode())
    n = d.n_seg
    return dict(dof=d.dof, seg_joint=[d.seg_joint[i] for i in range(n)], seg_xyz=[list(d.seg_xyz[i]) for i in range(n)],
                seg_R=[list(d.seg_R[i]) for i in range(n)], seg_axis=[list(d.seg_axis[i]) for i in range(n)],
                lower=lo[: d.dof].copy(), upper=up[: d.dof].copy())


def make_desc(*, kind, nb_deriv, horizon, dt, R_diag, chain, kp_timesteps, kp_Q, limits=None, kp_dist=None, kp_frames=None, kp_Ru=None,
              limit_multiplicity=1, kp_joint=None, limits2=None) -> ProblemDesc:
    """chain: dict(seg_joint, seg_xyz, seg_R, seg_axis, dof); limits: dict(state_max, state_min, limit_weight, penalty) or None."""
    L = load()
    d = ProblemDesc()
    L.ilqr_desc_defaults(C.byref(d))
    d.kind, d.nb_deriv, d.dof, d.horizon, d.dt = int(kind), int(nb_deriv), int(chain["dof"]), int(horizon), float(dt or 0.0)
    for i, v in enumerate(R_diag):
        d.R_diag[i] = float(v)
    n = len(chain["seg_joint"])
    if n > MAX_SEG:
        raise ValueError("too many segments")
    d.n_seg = n
    for i in range(n):
        d.seg_joint[i] = int(chain["seg_joint"][i])
        for k in range(3):
            d.seg_xyz[i][k] = float(chain["seg_xyz"][i][k])
            d.seg_axis[i][k] = float(chain["seg_axis"][i][k])
        for k in range(9):
            d.seg_R[i][k] = float(chain["seg_R"][i][k])
    dims = Dims()
    if L.ilqr_dims_of(C.byref(d), C.byref(dims)):
        raise ValueError("unsupported system kind / nb_deriv")
    if limits is not None:
        d.limits_set, d.penalty = 1, float(limits.get("penalty", 1.0))
        for i in range(len(limits["state_max"])):
            d.state_max[i] = float(limits["state_max"][i])
            d.state_min[i] = float(limits["state_min"][i])
            d.limit_weight[i] = int(limits["limit_weight"][i])
    d.n_kp = len(kp_timesteps)
    nq = dims.n_Q
    for k, (ts, Q) in enumerate(zip(kp_timesteps, kp_Q)):
        d.kp_timestep[k] = int(ts)
        jk = bool(kp_joint and kp_joint[k])  # Angular(Time)Keypoint of a joint-space sub-system (hybrid sequence): n_x x n_x precision
        d.kp_joint[k] = int(jk)
        nqk = dims.n_x if jk else nq
        Q = _f64(Q, (nqk, nqk))
        for a in range(nqk):
            for b in range(nqk):
                d.kp_Q[k][a * nqk + b] = Q[a, b]
    d.limit_multiplicity = int(limit_multiplicity)  # SequentialSystem: number of sub-systems
    if limits2 is not None:  # second group of sub-systems with other bounds: dict(state_max, state_min, limit_weight[, penalty, multiplicity])
        d.is_sequence, d.limits2_set, d.penalty2 = 1, 1, float(limits2.get("penalty", 1.0))
        d.limit_multiplicity2 = int(limits2.get("multiplicity", 1))
        for i in range(len(limits2["state_max"])):
            d.state_max2[i] = float(limits2["state_max"][i])
            d.state_min2[i] = float(limits2["state_min"][i])
            d.limit_weight2[i] = int(limits2["limit_weight"][i])
    for k, fr in enumerate(kp_frames or []):  # 4x4 pose of the object frame of keypoint k's sub-system (TransformedSimulationInterface) or None
        if fr is not None:
            Tm = _f64(fr, (4, 4))
            d.kp_has_frame[k] = 1
            for a in range(3):
                d.kp_frame_p[k][a] = Tm[a, 3]
                for b in range(3):
                    d.kp_frame_R[k][a * 3 + b] = Tm[a, b]
    for k, ru in enumerate(kp_Ru or []):  # control penalty of keypoint k's own sub-system (SequentialSystem) or None
        if ru is not None:
            d.kp_has_Ru[k] = 1
            for a, v in enumerate(ru):
                d.kp_Ru[k][a] = float(v)
    for k, kd in enumerate(kp_dist or []):  # PosOrnKeypointDistFunct: None or dict(pos_radius=..., orn_thresh=[3])
        if kd is not None:
            d.kp_dist[k] = 1
            d.kp_pos_radius[k] = float(kd["pos_radius"])
            for i in range(3):
                d.kp_orn_thresh[k][i] = float(kd["orn_thresh"][i])
    return d


class Context:
    def __init__(self, device_id: int = 0):
        import weakref

        self.L = load()
        self.h = C.c_void_p()
        self._problems = weakref.WeakSet()
        self.obstacle_path = 0  # what set_obstacle_path last set (the C side has no getter)
        rc = self.L.ilqr_ctx_create(device_id, C.byref(self.h))
        if rc:
            raise RuntimeError(f"ilqr_ctx_create failed (code {rc}): no usable HIP device {device_id}; there is no CPU fallback")

    def check(self, rc):
        if rc:
            raise RuntimeError(self.L.ilqr_last_error(self.h).decode())

    def set_stream(self, stream_ptr):
        self.check(self.L.ilqr_ctx_set_stream(self.h, C.c_void_p(stream_ptr)))

    def synchronize(self):
        self.check(self.L.ilqr_ctx_synchronize(self.h))

    _PINS = {"sweep": {None: 0, "mfma": 1, "rows": 2, "siwave": 4, "siwg": 5, "siwgio": 6, "siwgprep": 7}, "forward": {None: 0, "wg": 1, "dpp": 2, "wglds": 3, "wgio": 4}, "reroll": {None: 0, "rows": 1, "dpp": 2}}  # ILQR_XC_*

    def set_crosscheck(self, generic_kernels=False, cp_lane_solve=False, cp_general=False, sweep=None, forward=None, reroll=None):
        """Cross-check kernel variants (ilqr_ctx_set_crosscheck); context state, in force until changed.  sweep "mfma"|"rows"|"siwave"|"siwg"|"siwgio"|"siwgprep", forward "wg"|"dpp"|"wglds"|"wgio",
        reroll "rows"|"dpp"; None = by batch size."""
        pins = []
        for name, v in (("sweep", sweep), ("forward", forward), ("reroll", reroll)):
            if v not in self._PINS[name]:
                raise ValueError(f"set_crosscheck: {name} must be one of {[k for k in self._PINS[name] if k]} or None (got {v!r})")
            pins.append(self._PINS[name][v])
        self.check(self.L.ilqr_ctx_set_crosscheck(self.h, int(bool(generic_kernels)), int(bool(cp_lane_solve)), int(bool(cp_general)), *pins))

    def crosscheck_from_env(self):
        """TEST PLUMBING of this Python wrapper (the library itself reads no environment variable): the parity tests select the cross-check
        variants per test case through ILQR_HIP_PATH=v1, ILQR_CP_SOLVE=lane, ILQR_CP=general, ILQR_SWEEP=mfma|rows|siwave|siwg|siwgio|siwgprep, ILQR_FWD=wg|dpp|wglds|wgio, ILQR_APPLY=rows|dpp; every solve of BatchProblem passes them on."""
        env = os.environ
        self.set_crosscheck(env.get("ILQR_HIP_PATH") == "v1", env.get("ILQR_CP_SOLVE") == "lane", env.get("ILQR_CP") == "general",
                            sweep=env.get("ILQR_SWEEP") or None, forward=env.get("ILQR_FWD") or None, reroll=env.get("ILQR_APPLY") or None)

    OBSTACLE_PATHS = {"generic": 0, "cooperative": 1}  # ILQR_OBSTACLE_PATH_*

    def set_obstacle_path(self, path):
        """Kernel path of problems with obstacle terms (ilqr_ctx_set_obstacle_path): "generic" (the default) or "cooperative" (the cooperative
        kernels of the single-integrator systems, where the plan supports them), or the constant's integer; context state of its own, in force
        until changed -- set_crosscheck / crosscheck_from_env do not touch it.  Anything else is refused."""
        if isinstance(path, str):
            if path not in self.OBSTACLE_PATHS:
                raise ValueError(f"set_obstacle_path: path must be one of {list(self.OBSTACLE_PATHS)} (got {path!r})")
            path = self.OBSTACLE_PATHS[path]
        self.check(self.L.ilqr_ctx_set_obstacle_path(self.h, int(path)))
        self.obstacle_path = int(path)

    def set_split(self, mode: int):
        """Two-stream solve of large batches (ilqr_ctx_set_split): 0 off (one kernel at a time, for profiler runs), 1 where it was measured to pay
        (default), 2 every cooperative path (experiments); any other value raises."""
        self.check(self.L.ilqr_ctx_set_split(self.h, int(mode)))

    def profile(self, on: bool):
        self.check(self.L.ilqr_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self.check(self.L.ilqr_profile_reset(self.h))

    def profile_get(self, which):
        ms, n = C.c_double(), C.c_int()
        self.check(self.L.ilqr_profile_get(self.h, which, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def fk_batch(self, desc: ProblemDesc, q):
        q = _f64(q)
        n, dof = q.shape
        pos, quat, jac = np.zeros((n, 3)), np.zeros((n, 4)), np.zeros((n, 6, dof))
        self.check(self.L.ilqr_fk_batch(self.h, C.byref(desc), n, _dp(q), _dp(pos), _dp(quat), _dp(jac)))
        return pos, quat, jac

    def clearance_trajectories(self, desc: ProblemDesc, X, robot: ClrRobot, obstacles=None, traj_per_set=None, margin: float = 0.0, stats_group=None,
                               want=CLR_OUTPUTS):
        """Clearance of the trajectories X [n][T][n_x] (natural layout of desc) from the obstacles [n_sets][n_obs][4] and the robot's planes
        (ilqr_clearance_trajectories).  traj_per_set: None = one world for all; stats_group: asks for `stats`.  Returns a Clearance; what is not
        named in `want` is None."""
        X = _f64(X)
        n, T = X.shape[0], X.shape[1]
        want = tuple(want) + (("stats",) if stats_group is not None else ())
        return _clr_host_call(lambda r, w, o: self.check(self.L.ilqr_clearance_trajectories(self.h, C.byref(desc), n, T, X.ctypes.data, r, w, o)),
                              n, T, robot, obstacles, n if traj_per_set is None else traj_per_set, margin, stats_group, want)

    def clearance_trajectories_dev(self, desc: ProblemDesc, n: int, T: int, X_ptr, robot: ClrRobot, world: ClrWorld, out: ClrOut):
        """Device pointers in X_ptr, world.obs and out; asynchronous on the context's stream."""
        self.check(self.L.ilqr_clearance_trajectories_dev(self.h, C.byref(desc), int(n), int(T), X_ptr, C.byref(robot), C.byref(world), C.byref(out)))

    def close(self):
        if self.h:
            for p in list(self._problems):
                p.close()
            self.L.ilqr_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchProblem:
    """B instances of one lowered System (ilqr_problem)."""

    def __init__(self, ctx: Context, desc: ProblemDesc, batch: int):
        self.ctx, self.L, self.desc, self.B = ctx, ctx.L, desc, int(batch)
        self.dims = Dims()
        self.L.ilqr_dims_of(C.byref(desc), C.byref(self.dims))
        self.T, self.n_kp = desc.horizon, int(desc.n_kp)
        self.h = C.c_void_p()
        ctx.check(self.L.ilqr_problem_create(ctx.h, C.byref(desc), self.B, C.byref(self.h)))
        ctx._problems.add(self)
        self.m = 0

    # ---- inputs (host arrays)
    def set_init_state(self, q0, dq0=None):
        q0 = _f64(q0, (self.B, self.desc.dof))
        dq0 = _f64(dq0, (self.B, self.desc.dof)) if dq0 is not None else None
        self.ctx.check(self.L.ilqr_problem_set_init_state(self.h, q0.ctypes.data, dq0.ctypes.data if dq0 is not None else None))

    def set_keypoint_targets(self, k, target):
        t = _f64(target, (self.B, self.dims.n_f))
        self.ctx.check(self.L.ilqr_problem_set_keypoint_targets(self.h, k, t.ctypes.data))

    def set_controls(self, U0):
        U0 = _f64(U0, (self.B, self.T - 1, self.dims.n_u))
        self.ctx.check(self.L.ilqr_problem_set_controls(self.h, U0.ctypes.data))

    def set_constraints(self, A, b, lambda0=None):
        A, b = _f64(A), _f64(b)
        per_step = 1 if A.ndim == 3 else 0
        self.m = A.shape[-2]
        lam = _f64(lambda0, (self.B, self.T - 1, self.m)) if lambda0 is not None else None
        self.ctx.check(self.L.ilqr_problem_set_constraints(self.h, self.m, per_step, _dp(A), _dp(b), _dp(lam)))

    def reset_multipliers(self):
        self.ctx.check(self.L.ilqr_problem_reset_multipliers(self.h))

    # ---- inputs (device pointers, e.g. tensor.data_ptr())
    def set_init_state_dev(self, q0_ptr, dq0_ptr=None):
        self.ctx.check(self.L.ilqr_problem_set_init_state_dev(self.h, q0_ptr, dq0_ptr))

    def set_keypoint_targets_dev(self, k, ptr):
        self.ctx.check(self.L.ilqr_problem_set_keypoint_targets_dev(self.h, k, ptr))

    def set_controls_dev(self, ptr):
        self.ctx.check(self.L.ilqr_problem_set_controls_dev(self.h, ptr))

    # ---- solvers (asynchronous on the context's stream)
    def solve_recursive(self, nb_iter, line_search=True, early_stop=True):
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_solve_recursive(self.h, nb_iter, int(line_search), int(early_stop)))

    def solve_al(self, nb_iter, lag_update_step, penalty, scaling_factor, line_search=True, early_stop=True):
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_solve_al(self.h, nb_iter, lag_update_step, penalty, scaling_factor, int(line_search), int(early_stop)))

    def solve_batch_cp(self, psi, nb_iter, early_stop=True):
        psi = _f64(psi)
        assert psi.shape[0] == (self.T - 1) * self.dims.n_u
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_solve_batch_cp(self.h, _dp(psi), psi.shape[1], nb_iter, int(early_stop)))

    def solve_batch(self, nb_iter, early_stop=True):
        """BatchILQR::solve: the batch solver on the full control sequence (identity basis)."""
        self.ctx.check(self.L.ilqr_solve_batch(self.h, nb_iter, int(early_stop)))

    # ---- results
    def _get(self, name, shape):
        o = np.zeros(shape)
        self.ctx.check(getattr(self.L, "ilqr_problem_get_" + name)(self.h, o.ctypes.data))
        return o

    def X(self):
        return self._get("X", (self.B, self.T, self.dims.n_x))

    def fX(self):
        return self._get("fX", (self.B, self.T, self.dims.n_f))

    def U(self):
        return self._get("U", (self.B, self.T - 1, self.dims.n_u))

    def K(self):
        return self._get("K", (self.B, self.T - 1, self.dims.n_u, self.dims.n_x))

    def d(self):
        return self._get("d", (self.B, self.T - 1, self.dims.n_u))

    def cost(self):
        return self._get("cost", (self.B,))

    def alpha(self):
        return self._get("alpha", (self.B,))

    def lam(self):
        return self._get("lambda", (self.B, self.T - 1, self.m))

    def iters(self):
        o = np.zeros(self.B, dtype=np.int32)
        self.ctx.check(self.L.ilqr_problem_get_iters(self.h, o.ctypes.data_as(C.POINTER(C.c_int))))
        return o

    def status(self):
        o = np.zeros(self.B, dtype=np.int32)
        self.ctx.check(self.L.ilqr_problem_get_status(self.h, o.ctypes.data_as(C.POINTER(C.c_int))))
        return o

    def trace(self, nb_iter):
        ct, at = np.zeros((self.B, nb_iter)), np.zeros((self.B, nb_iter))
        self.ctx.check(self.L.ilqr_problem_get_trace(self.h, _dp(ct), _dp(at), nb_iter))
        return ct, at

    def get_X_dev(self, ptr):
        self.ctx.check(self.L.ilqr_problem_get_X_dev(self.h, ptr))

    def get_U_dev(self, ptr):
        self.ctx.check(self.L.ilqr_problem_get_U_dev(self.h, ptr))

    def get_cost_dev(self, ptr):
        self.ctx.check(self.L.ilqr_problem_get_cost_dev(self.h, ptr))

    # ---- receding horizon / tracking
    def warm_start(self, shift: int = 0):
        self.ctx.check(self.L.ilqr_problem_warm_start(self.h, int(shift)))

    def gains(self):
        """Gains about the plan the problem holds (ilqr_problem_gains): one backward sweep about X(), U(), whichever solver left them -- the batch
        solvers and a 0-iteration solve_recursive included.  Afterwards K(), d() are that sweep's (d unscaled, alpha() all ones) and track and the
        closed-loop calls run on them; X, U, cost, iters, status, lam and the trace are untouched.  Asynchronous on the context's stream."""
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_gains(self.h))

    def gains_al(self, penalty: float):
        """gains() with the augmented-Lagrangian terms of the constraint rows (ilqr_problem_gains_al): the AL sweep about X(), U() with the active-set
        weights penalty * I of that plan and the multipliers lam() as they are; no multiplier moves.  `penalty`: the one the plan's solve ended
        with, or any other finite value >= 0."""
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_gains_al(self.h, float(penalty)))

    def track(self, k: int, x_meas, with_feedforward: bool = False):
        x = _f64(x_meas, (self.B, self.dims.n_x))
        u = np.empty((self.B, self.dims.n_u))
        self.ctx.check(self.L.ilqr_problem_track(self.h, int(k), _dp(x), int(bool(with_feedforward)), _dp(u)))
        return u

    def _cl_inputs(self, samples, x0, w=None):
        """(S, n, x0, w) of a closed-loop call: S is `samples`, else what x0 or w gives, else 1; n = max(S, 0) sizes the arrays (the library
        refuses S < 1; they must merely exist); x0 and w are coerced to their shapes."""
        S = samples
        for arr in (x0, w):
            if S is None and arr is not None:
                S = np.shape(arr)[1]
        S = 1 if S is None else int(S)
        n = max(S, 0)
        x0 = _f64(x0, (self.B, n, self.dims.n_x)) if x0 is not None else None
        w = _f64(w, (self.B, n, self.T - 1, self.dims.n_x)) if w is not None else None
        return S, n, x0, w

    def closed_loop(self, x0=None, w=None, samples=None, with_feedforward: bool = False, want_X: bool = True, want_U: bool = True):
        """Closed loop of the tracking law on the last Riccati solve's plan (ilqr_problem_closed_loop): x0 [B][S][n_x] or None (the plan's start),
        w [B][S][T-1][n_x] or None (no disturbance); samples: S, needed only where neither array gives it.  Returns (cost [B][S],
        X [B][S][T][n_x] or None, U [B][S][T-1][n_u] or None)."""
        S, n, x0, w = self._cl_inputs(samples, x0, w)
        cost = np.empty((self.B, n))
        X, U = _out(want_X, self.B, n, self.T, self.dims.n_x), _out(want_U, self.B, n, self.T - 1, self.dims.n_u)
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop(self.h, S, _dp(x0), _dp(w), int(bool(with_feedforward)), _dp(cost), _dp(X), _dp(U)))
        return cost, X, U

    def closed_loop_dev(self, samples: int, x0_ptr, w_ptr, with_feedforward: bool, cost_ptr, X_ptr=None, U_ptr=None):
        """Device pointers (0 / None where ilqr_problem_closed_loop takes NULL), asynchronous on the context's stream."""
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop_dev(self.h, int(samples), x0_ptr or None, w_ptr or None, int(bool(with_feedforward)),
                                                           cost_ptr or None, X_ptr or None, U_ptr or None))

    def noise(self, seed, sigma_w=None, sigma_x0=None, instance_offset=0, sample_offset=0):
        """The ilqr_noise of a call: sigma_w / sigma_x0 a scalar (every entry) or n_x values in the user's state layout, None = 0."""
        nz = Noise()
        nz.seed, nz.instance_offset, nz.sample_offset = int(seed), int(instance_offset), int(sample_offset)
        for field, sig in ((nz.sigma_w, sigma_w), (nz.sigma_x0, sigma_x0)):
            v = np.broadcast_to(np.asarray(0.0 if sig is None else sig, dtype=np.float64), (self.dims.n_x,))
            for i in range(self.dims.n_x):
                field[i] = v[i]
        return nz

    def closed_loop_noise(self, samples, seed, sigma_w=None, sigma_x0=None, x0=None, with_feedforward: bool = False, instance_offset=0,
                          sample_offset=0, want_cost: bool = True, want_stats: bool = True, want_X: bool = False, want_U: bool = False,
                          want_w: bool = False):
        """The closed loop with its disturbances sigma_w z and start perturbations sigma_x0 z drawn on the device (ilqr_problem_closed_loop_noise):
        the draw of (seed, instance_offset + b, sample_offset + s, step, entry) is the definition in include/ilqr_hip.h.  x0 [B][S][n_x] or None
        is the centre of the start perturbation.  Returns a ClosedLoopNoise of cost [B][S], stats [B][5] (mean, variance, min, max of the
        finite costs, n_bad), X, U, w [B][S][T-1][n_x]; what was not asked for is None."""
        S, n, x0, _ = self._cl_inputs(int(samples), x0)
        cost, stats = _out(want_cost, self.B, n), _out(want_stats, self.B, CL_STATS)
        X, U = _out(want_X, self.B, n, self.T, self.dims.n_x), _out(want_U, self.B, n, self.T - 1, self.dims.n_u)
        w = _out(want_w, self.B, n, self.T - 1, self.dims.n_x)
        nz = self.noise(seed, sigma_w, sigma_x0, instance_offset, sample_offset)
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop_noise(self.h, S, C.byref(nz), _dp(x0), int(bool(with_feedforward)), _dp(cost), _dp(stats),
                                                             _dp(X), _dp(U), _dp(w)))
        return ClosedLoopNoise(cost, stats, X, U, w)

    def closed_loop_noise_dev(self, samples: int, noise, x0_ptr, with_feedforward: bool, cost_ptr=None, stats_ptr=None, X_ptr=None, U_ptr=None,
                              w_ptr=None):
        """Device pointers (0 / None where ilqr_problem_closed_loop_noise takes NULL), asynchronous on the context's stream; noise: self.noise(..)."""
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop_noise_dev(self.h, int(samples), C.byref(noise) if noise is not None else None, x0_ptr or None,
                                                                 int(bool(with_feedforward)), cost_ptr or None, stats_ptr or None, X_ptr or None,
                                                                 U_ptr or None, w_ptr or None))

    def tol(self, kp_tol=None, lim_tol=0.0):
        """The ilqr_cl_tol of a report: kp_tol a scalar (every keypoint and group), 5 values (every keypoint) or [n_kp][5]; negative = that group
        is not judged, None = nothing is judged.  lim_tol >= 0."""
        t = Tol()
        v = np.broadcast_to(np.asarray(-1.0 if kp_tol is None else kp_tol, dtype=np.float64), (self.n_kp, KP_ERR))
        for k in range(MAX_KP):
            for g in range(KP_ERR):
                t.kp_tol[k][g] = v[k, g] if k < self.n_kp else -1.0
        t.lim_tol = float(lim_tol)
        return t

    def closed_loop_report(self, samples=None, seed=None, sigma_w=None, sigma_x0=None, x0=None, w=None, with_feedforward: bool = False,
                           kp_tol=None, lim_tol=None, instance_offset=0, sample_offset=0, want_cost: bool = True, want_stats: bool = True,
                           want_kp_err: bool = True, want_kp_stats: bool = True, want_lim_cost: bool = True, want_outcome: bool = True,
                           want_X: bool = False, want_U: bool = False, want_w: bool = False):
        """The closed loop with a report of what every execution did (ilqr_problem_closed_loop_report; definitions in include/ilqr_hip.h):
        kp_err [B][S][n_kp][5] (pos, orn, vel, angvel, time), kp_stats [B][n_kp][12] (mean[5], max[5], n_miss, n_bad), lim_cost [B][S] and
        outcome [B][4] (n_ok, n_miss, n_lim, n_bad).  seed given: the draw of closed_loop_noise (x0 its centre); w given: the caller's
        disturbances; neither: none.  kp_tol: see tol(); with kp_tol and lim_tol both None no tolerance is passed and the two reductions are
        not asked for.  X, U, w are not outputs of the C call: where they are wanted they come from closed_loop_noise / closed_loop with the same
        inputs, which run the same rollout bit for bit.  Returns a ClosedLoopReport; what was not asked for is None."""
        S, n, x0, w = self._cl_inputs(samples, x0, w)
        nz = self.noise(seed, sigma_w, sigma_x0, instance_offset, sample_offset) if seed is not None else None
        judged = kp_tol is not None or lim_tol is not None
        tol = self.tol(kp_tol, 0.0 if lim_tol is None else lim_tol) if judged else None
        cost, stats = _out(want_cost, self.B, n), _out(want_stats, self.B, CL_STATS)
        kp_err, kp_stats = _out(want_kp_err, self.B, n, self.n_kp, KP_ERR), _out(want_kp_stats and judged, self.B, self.n_kp, KP_STATS)
        lim_cost, outcome = _out(want_lim_cost, self.B, n), _out(want_outcome and judged, self.B, CL_OUTCOME)
        rp = Report(*(a.ctypes.data if a is not None else None for a in (kp_err, kp_stats, lim_cost, outcome)))
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop_report(self.h, S, C.byref(nz) if nz is not None else None, _dp(x0), _dp(w),
                                                              int(bool(with_feedforward)), C.byref(tol) if tol is not None else None, _dp(cost),
                                                              _dp(stats), C.byref(rp)))
        X = U = wo = None
        if want_X or want_U or want_w:
            if nz is not None:
                r = self.closed_loop_noise(S, seed, sigma_w, sigma_x0, x0, with_feedforward, instance_offset, sample_offset, want_stats=False,
                                           want_X=want_X, want_U=want_U, want_w=want_w)
                X, U, wo = r.X, r.U, r.w
            else:
                _, X, U = self.closed_loop(x0, w, S, with_feedforward, want_X=want_X, want_U=want_U)
                wo = w if want_w else None
        return ClosedLoopReport(cost, stats, kp_err, kp_stats, lim_cost, outcome, X, U, wo)

    def closed_loop_report_dev(self, samples: int, noise, x0_ptr, w_ptr, with_feedforward: bool, tol, cost_ptr=None, stats_ptr=None,
                               kp_err_ptr=None, kp_stats_ptr=None, lim_cost_ptr=None, outcome_ptr=None):
        """Device pointers (0 / None where ilqr_problem_closed_loop_report takes NULL), asynchronous on the context's stream; noise: self.noise(..)
        or None, tol: self.tol(..) or None."""
        rp = Report(kp_err_ptr or None, kp_stats_ptr or None, lim_cost_ptr or None, outcome_ptr or None)
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop_report_dev(self.h, int(samples), C.byref(noise) if noise is not None else None,
                                                                  x0_ptr or None, w_ptr or None, int(bool(with_feedforward)),
                                                                  C.byref(tol) if tol is not None else None, cost_ptr or None, stats_ptr or None,
                                                                  C.byref(rp)))

    def closed_loop_report_con(self, con_tol, samples=None, seed=None, sigma_w=None, sigma_x0=None, x0=None, w=None, with_feedforward: bool = False,
                               kp_tol=None, lim_tol=None, instance_offset=0, sample_offset=0, want_cost: bool = True, want_stats: bool = True,
                               want_kp_err: bool = True, want_kp_stats: bool = True, want_lim_cost: bool = True, want_outcome: bool = True,
                               want_con_max: bool = True, want_con_steps: bool = True, want_con_stats: bool = True, want_outcome_con: bool = True):
        """closed_loop_report with the executions judged against the rows of set_constraints as well (ilqr_problem_closed_loop_report_con;
        definitions in include/ilqr_hip.h): con_max [B][S], con_steps [B][S], con_stats [B][6] (mean con_max, max con_max, mean con_steps, max
        con_steps, n_con, n_bad) and, with kp_tol or lim_tol, outcome_con [B][5] (n_ok, n_miss, n_lim, n_con, n_bad).  One rollout; the other
        arguments and outputs are closed_loop_report's.  Returns a ClosedLoopReportCon; what was not asked for is None."""
        S, n, x0, w = self._cl_inputs(samples, x0, w)
        nz = self.noise(seed, sigma_w, sigma_x0, instance_offset, sample_offset) if seed is not None else None
        judged = kp_tol is not None or lim_tol is not None
        tol = self.tol(kp_tol, 0.0 if lim_tol is None else lim_tol) if judged else None
        cost, stats = _out(want_cost, self.B, n), _out(want_stats, self.B, CL_STATS)
        kp_err, kp_stats = _out(want_kp_err, self.B, n, self.n_kp, KP_ERR), _out(want_kp_stats and judged, self.B, self.n_kp, KP_STATS)
        lim_cost, outcome = _out(want_lim_cost, self.B, n), _out(want_outcome and judged, self.B, CL_OUTCOME)
        con_max, con_steps = _out(want_con_max, self.B, n), _out(want_con_steps, self.B, n)
        con_stats, outcome_con = _out(want_con_stats, self.B, CL_CON_STATS), _out(want_outcome_con and judged, self.B, CL_OUTCOME_CON)
        rp = Report(*(a.ctypes.data if a is not None else None for a in (kp_err, kp_stats, lim_cost, outcome)))
        co = Con(*(a.ctypes.data if a is not None else None for a in (con_max, con_steps, con_stats, outcome_con)))
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop_report_con(self.h, S, C.byref(nz) if nz is not None else None, _dp(x0), _dp(w),
                                                                  int(bool(with_feedforward)), C.byref(tol) if tol is not None else None, _dp(cost),
                                                                  _dp(stats), C.byref(rp), float(con_tol), C.byref(co)))
        return ClosedLoopReportCon(cost, stats, kp_err, kp_stats, lim_cost, outcome, con_max, con_steps, con_stats, outcome_con)

    def closed_loop_report_con_dev(self, samples: int, noise, x0_ptr, w_ptr, with_feedforward: bool, tol, con_tol, cost_ptr=None, stats_ptr=None,
                                   kp_err_ptr=None, kp_stats_ptr=None, lim_cost_ptr=None, outcome_ptr=None, con_max_ptr=None, con_steps_ptr=None,
                                   con_stats_ptr=None, outcome_con_ptr=None):
        """Device pointers (0 / None where ilqr_problem_closed_loop_report_con takes NULL), asynchronous on the context's stream; noise:
        self.noise(..) or None, tol: self.tol(..) or None."""
        rp = Report(kp_err_ptr or None, kp_stats_ptr or None, lim_cost_ptr or None, outcome_ptr or None)
        co = Con(con_max_ptr or None, con_steps_ptr or None, con_stats_ptr or None, outcome_con_ptr or None)
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop_report_con_dev(self.h, int(samples), C.byref(noise) if noise is not None else None,
                                                                      x0_ptr or None, w_ptr or None, int(bool(with_feedforward)),
                                                                      C.byref(tol) if tol is not None else None, cost_ptr or None, stats_ptr or None,
                                                                      C.byref(rp), float(con_tol), C.byref(co)))

    def _sigma(self, sig):
        """A sigma of a covariance call: None (zeros, passed as NULL), a scalar (every entry) or n_x values in the user's state layout."""
        return None if sig is None else np.ascontiguousarray(np.broadcast_to(np.asarray(sig, dtype=np.float64), (self.dims.n_x,)))

    def closed_loop_cov(self, sigma_w=None, sigma_x0=None, want_Sigma: bool = False, want_kp_Sigma: bool = True, want_kp_var: bool = True,
                        want_u_var: bool = True, want_lim_z: bool = True):
        """The state covariance of the closed loop under the noise model of closed_loop_noise, propagated analytically on the device
        (ilqr_problem_closed_loop_cov; definitions in include/ilqr_hip.h): Sigma [B][T][n_x][n_x], kp_Sigma [B][n_kp][n_x][n_x], kp_var
        [B][n_kp][5] (pos, orn, vel, angvel, time), u_var [B][T-1][n_u], lim_z [B].  Returns a ClosedLoopCov; what was not asked for is None."""
        nx = self.dims.n_x
        Sigma, kp_Sigma = _out(want_Sigma, self.B, self.T, nx, nx), _out(want_kp_Sigma, self.B, self.n_kp, nx, nx)
        kp_var, u_var = _out(want_kp_var, self.B, self.n_kp, KP_ERR), _out(want_u_var, self.B, self.T - 1, self.dims.n_u)
        lim_z = _out(want_lim_z, self.B)
        cv = Cov(*(a.ctypes.data if a is not None else None for a in (Sigma, kp_Sigma, kp_var, u_var, lim_z)))
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop_cov(self.h, _dp(self._sigma(sigma_w)), _dp(self._sigma(sigma_x0)), C.byref(cv)))
        return ClosedLoopCov(Sigma, kp_Sigma, kp_var, u_var, lim_z)

    def closed_loop_cov_dev(self, sigma_w=None, sigma_x0=None, Sigma_ptr=None, kp_Sigma_ptr=None, kp_var_ptr=None, u_var_ptr=None, lim_z_ptr=None):
        """Device pointers (0 / None where the output is not asked for), asynchronous on the context's stream; the sigmas are host values."""
        cv = Cov(Sigma_ptr or None, kp_Sigma_ptr or None, kp_var_ptr or None, u_var_ptr or None, lim_z_ptr or None)
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop_cov_dev(self.h, _dp(self._sigma(sigma_w)), _dp(self._sigma(sigma_x0)), C.byref(cv)))

    def closed_loop_cov_con(self, sigma_w=None, sigma_x0=None, want_Sigma: bool = False, want_kp_Sigma: bool = False, want_kp_var: bool = False,
                            want_u_var: bool = False, want_lim_z: bool = False, want_con_var: bool = True, want_con_z: bool = True):
        """closed_loop_cov with the rows of set_constraints read off the same recursion (ilqr_problem_closed_loop_cov_con; definitions in
        include/ilqr_hip.h): con_var [B][T-1][m], the first-order variance of every row at every control step, and con_z [B], how many standard
        deviations the plan keeps from its constraints.  Returns a ClosedLoopCovCon; what was not asked for is None."""
        nx = self.dims.n_x
        Sigma, kp_Sigma = _out(want_Sigma, self.B, self.T, nx, nx), _out(want_kp_Sigma, self.B, self.n_kp, nx, nx)
        kp_var, u_var = _out(want_kp_var, self.B, self.n_kp, KP_ERR), _out(want_u_var, self.B, self.T - 1, self.dims.n_u)
        lim_z = _out(want_lim_z, self.B)
        con_var, con_z = _out(want_con_var, self.B, self.T - 1, max(self.m, 0)), _out(want_con_z, self.B)
        cv = Cov(*(a.ctypes.data if a is not None else None for a in (Sigma, kp_Sigma, kp_var, u_var, lim_z)))
        co = CovCon(*(a.ctypes.data if a is not None else None for a in (con_var, con_z)))
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop_cov_con(self.h, _dp(self._sigma(sigma_w)), _dp(self._sigma(sigma_x0)), C.byref(cv), C.byref(co)))
        return ClosedLoopCovCon(Sigma, kp_Sigma, kp_var, u_var, lim_z, con_var, con_z)

    def closed_loop_cov_con_dev(self, sigma_w=None, sigma_x0=None, Sigma_ptr=None, kp_Sigma_ptr=None, kp_var_ptr=None, u_var_ptr=None, lim_z_ptr=None,
                                con_var_ptr=None, con_z_ptr=None):
        """Device pointers (0 / None where the output is not asked for), asynchronous on the context's stream; the sigmas are host values."""
        cv = Cov(Sigma_ptr or None, kp_Sigma_ptr or None, kp_var_ptr or None, u_var_ptr or None, lim_z_ptr or None)
        co = CovCon(con_var_ptr or None, con_z_ptr or None)
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop_cov_con_dev(self.h, _dp(self._sigma(sigma_w)), _dp(self._sigma(sigma_x0)), C.byref(cv), C.byref(co)))

    def closed_loop_cov_clr(self, sigma_w, sigma_x0, robot: ClrRobot, world, z_tol: float = 0.0, want=COV_CLR_OUTPUTS):
        """closed_loop_cov with the clearance pairs read off the same recursion (ilqr_problem_closed_loop_cov_clr; definitions in
        include/ilqr_hip.h): clr_var, clr_z [B][T], clr_z_min [B], clr_z_at [B][3] (int32) and eligible [B] (int32).  robot: clr_robot(...);
        world: a ClrWorld whose obs is a host pointer, or (obstacles [n_sets][n_obs][4] or None, traj_per_set or None for B, margin).  want:
        names of COV_CLR_OUTPUTS and of the five covariance outputs ("Sigma", "kp_Sigma", "kp_var", "u_var", "lim_z").  Returns a
        ClosedLoopCovClr; what was not asked for is None."""
        nx = self.dims.n_x
        if not isinstance(world, ClrWorld):
            obstacles, tps, margin = world
            tps = self.B if tps is None else int(tps)
            obs = _f64(obstacles) if obstacles is not None else np.zeros((self.B // tps if tps >= 1 else 0, 0, 4))
            if obs.ndim != 3 or obs.shape[2] != 4:
                raise ValueError(f"obstacles: expected [n_sets][n_obs][4], got {obs.shape}")
            world = ClrWorld(obs.ctypes.data if obs.size else None, obs.shape[0], obs.shape[1], tps, float(margin), 0)
        Sigma, kp_Sigma = _out("Sigma" in want, self.B, self.T, nx, nx), _out("kp_Sigma" in want, self.B, self.n_kp, nx, nx)
        kp_var, u_var = _out("kp_var" in want, self.B, self.n_kp, KP_ERR), _out("u_var" in want, self.B, self.T - 1, self.dims.n_u)
        lim_z = _out("lim_z" in want, self.B)
        var, z, zmin = _out("clr_var" in want, self.B, self.T), _out("clr_z" in want, self.B, self.T), _out("clr_z_min" in want, self.B)
        at = np.empty((self.B, 3), dtype=np.int32) if "clr_z_at" in want else None
        el = np.empty(self.B, dtype=np.int32) if "eligible" in want else None
        cv = Cov(*(a.ctypes.data if a is not None else None for a in (Sigma, kp_Sigma, kp_var, u_var, lim_z)))
        ck = ClCovClr(*(a.ctypes.data if a is not None else None for a in (var, z, zmin, at, el)))
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop_cov_clr(self.h, _dp(self._sigma(sigma_w)), _dp(self._sigma(sigma_x0)), C.byref(cv), C.byref(robot),
                                                               C.byref(world), float(z_tol), C.byref(ck)))
        return ClosedLoopCovClr(Sigma, kp_Sigma, kp_var, u_var, lim_z, var, z, zmin, at, el)

    def closed_loop_cov_clr_dev(self, sigma_w, sigma_x0, robot: ClrRobot, world: ClrWorld, z_tol: float, clr: ClCovClr, cov: Cov = None):
        """Device pointers in world.obs, clr and cov (cov may be None); asynchronous on the context's stream; the sigmas are host values."""
        self.ctx.crosscheck_from_env()
        self.ctx.check(self.L.ilqr_problem_closed_loop_cov_clr_dev(self.h, _dp(self._sigma(sigma_w)), _dp(self._sigma(sigma_x0)),
                                                                   C.byref(cov) if cov is not None else None, C.byref(robot), C.byref(world),
                                                                   float(z_tol), C.byref(clr) if clr is not None else None))

    # ---- multi-start: the calls that join instances (include/ilqr_hip.h "multi-start")
    @staticmethod
    def _i32(a, n=None):
        a = np.ascontiguousarray(np.asarray(a), dtype=np.int32)
        if a.ndim != 1 or (n is not None and a.shape[0] != n):
            raise ValueError(f"expected {n if n is not None else 'a vector of'} ints, got shape {a.shape}")
        return a

    def adopt(self, src: "BatchProblem", index, what: int):
        """Instance i of this problem takes from instance index[i] of `src` what the ADOPT_* bits of `what` name (ilqr_problem_adopt): device to
        device.  index: B ints in 0 .. src.B-1 (index[b] = b // S replicates G tasks over G * S instances)."""
        idx = self._i32(index, self.B)
        self.ctx.check(self.L.ilqr_problem_adopt(self.h, src.h, idx.ctypes.data, int(what)))

    def adopt_dev(self, src: "BatchProblem", index_ptr, what: int):
        """index_ptr: B ints in device memory (clamped into src's batch by the kernel); asynchronous on the context's stream."""
        self.ctx.check(self.L.ilqr_problem_adopt_dev(self.h, src.h, index_ptr, int(what)))

    def _seeds(self, seed, sigma_u, group_offset, member_offset):
        sd = Seeds(int(seed), int(group_offset), int(member_offset))
        for i, v in enumerate(np.broadcast_to(np.asarray(sigma_u, dtype=np.float64), (self.dims.n_u,))):
            sd.sigma_u[i] = float(v)
        return sd

    def spread_controls(self, group_size: int, seed: int, sigma_u, group_offset: int = 0, member_offset: int = 0):
        """The starts of every group of `group_size` instances (ilqr_problem_spread_controls): member 0 keeps its U0, every other member gets
        U0 += sigma_u * z; sigma_u: a scalar or n_u values in the user's control layout.  Asynchronous on the context's stream."""
        self.ctx.check(self.L.ilqr_problem_spread_controls(self.h, int(group_size), C.byref(self._seeds(seed, sigma_u, group_offset, member_offset))))

    def spread_controls_dev(self, group_size: int, seed: int, sigma_u, group_offset: int = 0, member_offset: int = 0):
        self.ctx.check(self.L.ilqr_problem_spread_controls_dev(self.h, int(group_size), C.byref(self._seeds(seed, sigma_u, group_offset, member_offset))))

    def select(self, group_size: int, score=None, eligible=None, want_winner: bool = True, want_best: bool = True, want_n_candidates: bool = True):
        """The best member of every group (ilqr_problem_select): score [B] or None (the cost), eligible [B] ints or None (all).  Returns a Selection
        (winner [G] int32, best [G], n_candidates [G] int32); what was not asked for is None."""
        G = self.B // int(group_size) if int(group_size) >= 1 else 0
        sc = _f64(score, (self.B,)) if score is not None else None
        el = self._i32(eligible, self.B) if eligible is not None else None
        win = np.empty(G, dtype=np.int32) if want_winner else None
        best = np.empty(G) if want_best else None
        nc = np.empty(G, dtype=np.int32) if want_n_candidates else None
        self.ctx.check(self.L.ilqr_problem_select(self.h, int(group_size), *(a.ctypes.data if a is not None else None for a in (sc, el, win, best, nc))))
        return Selection(win, best, nc)

    def select_dev(self, group_size: int, score_ptr=None, eligible_ptr=None, winner_ptr=None, best_ptr=None, n_candidates_ptr=None):
        """Device pointers (0 / None: the cost, all eligible, output not asked for); asynchronous on the context's stream."""
        self.ctx.check(self.L.ilqr_problem_select_dev(self.h, int(group_size), score_ptr or None, eligible_ptr or None, winner_ptr or None,
                                                      best_ptr or None, n_candidates_ptr or None))

    def get_at(self, index, want_X: bool = True, want_U: bool = True, want_cost: bool = True, want_iters: bool = True, want_status: bool = True):
        """Rows index[0 .. n-1] of X(), U(), cost(), iters(), status() (ilqr_problem_get_at).  Returns a Rows; what was not asked for is None."""
        idx = self._i32(index)
        n = idx.shape[0]
        X, U, cost = _out(want_X, n, self.T, self.dims.n_x), _out(want_U, n, self.T - 1, self.dims.n_u), _out(want_cost, n)
        it = np.empty(n, dtype=np.int32) if want_iters else None
        st = np.empty(n, dtype=np.int32) if want_status else None
        self.ctx.check(self.L.ilqr_problem_get_at(self.h, n, idx.ctypes.data, *(a.ctypes.data if a is not None else None for a in (X, U, cost, it, st))))
        return Rows(X, U, cost, it, st)

    def get_at_dev(self, n: int, index_ptr, X_ptr=None, U_ptr=None, cost_ptr=None, iters_ptr=None, status_ptr=None):
        """Device pointers (0 / None where the output is not asked for; indices clamped by the kernel); asynchronous on the context's stream."""
        self.ctx.check(self.L.ilqr_problem_get_at_dev(self.h, int(n), index_ptr, X_ptr or None, U_ptr or None, cost_ptr or None, iters_ptr or None,
                                                      status_ptr or None))

    # ---- clearance of the plan from sphere obstacles and planes (include/ilqr_hip.h "clearance")
    def clearance(self, robot: ClrRobot, obstacles=None, traj_per_set=None, margin: float = 0.0, stats_group=None, want=CLR_OUTPUTS):
        """Clearance of the plan this problem holds (ilqr_problem_clearance), read where it lies; arguments and result as
        Context.clearance_trajectories with n = B."""
        want = tuple(want) + (("stats",) if stats_group is not None else ())
        return _clr_host_call(lambda r, w, o: self.ctx.check(self.L.ilqr_problem_clearance(self.h, r, w, o)), self.B, self.T, robot, obstacles,
                              self.B if traj_per_set is None else traj_per_set, margin, stats_group, want)

    def clearance_dev(self, robot: ClrRobot, world: ClrWorld, out: ClrOut):
        """Device pointers in world.obs and out; asynchronous on the context's stream."""
        self.ctx.check(self.L.ilqr_problem_clearance_dev(self.h, C.byref(robot), C.byref(world), C.byref(out)))

    # ---- obstacle terms in the stage cost of the Riccati solvers (include/ilqr_hip.h "obstacle terms")
    def set_obstacles(self, spheres, planes, obstacles, margin: float, weight: float, traj_per_set=None, self_pairs=None):
        """Hinge penalty weight * max(0, margin - clearance)^2 on every (sphere, obstacle or plane) pair and every self pair at every step
        (ilqr_problem_set_obstacles).  spheres, planes, self_pairs as clr_robot takes them (or a ClrRobot in `spheres` with planes and self_pairs
        None); obstacles [n_sets][n_obs][4] or None (planes or self pairs only); traj_per_set: None = one world for all.  The problem copies
        everything; it holds no plan afterwards."""
        rb = spheres if isinstance(spheres, ClrRobot) else clr_robot(spheres, planes, self_pairs)
        tps = self.B if traj_per_set is None else int(traj_per_set)
        obs = _f64(obstacles) if obstacles is not None else np.zeros((self.B // tps if tps >= 1 else 0, 0, 4))
        if obs.ndim != 3 or obs.shape[2] != 4:
            raise ValueError(f"obstacles: expected [n_sets][n_obs][4], got {obs.shape}")
        w = ClrWorld(obs.ctypes.data if obs.size else None, obs.shape[0], obs.shape[1], tps, float(margin), 0)
        self.ctx.check(self.L.ilqr_problem_set_obstacles(self.h, C.byref(rb), C.byref(w), float(weight)))

    def set_obstacles_dev(self, robot: ClrRobot, world: ClrWorld, weight: float):
        """world.obs is a device pointer; the problem copies the sets device to device."""
        self.ctx.check(self.L.ilqr_problem_set_obstacles_dev(self.h, C.byref(robot), C.byref(world), float(weight)))

    def clear_obstacles(self):
        """Remove the obstacle terms: the problem is planned as before they were set (it holds no plan afterwards)."""
        self.ctx.check(self.L.ilqr_problem_set_obstacles(self.h, None, None, 0.0))

    def obstacle_terms(self, want=("cost", "lx", "lxx")):
        """c_obs[B][T], its l_x[B][T][dof] and l_xx[B][T][dof][dof] at the plan this problem holds (ilqr_problem_obstacle_terms); what is not
        wanted is None."""
        dof = int(self.desc.dof)
        cost, lx, lxx = _out("cost" in want, self.B, self.T), _out("lx" in want, self.B, self.T, dof), _out("lxx" in want, self.B, self.T, dof, dof)
        self.ctx.check(self.L.ilqr_problem_obstacle_terms(self.h, *(a.ctypes.data if a is not None else None for a in (cost, lx, lxx))))
        return ObstacleTerms(cost, lx, lxx)

    def obstacle_terms_dev(self, cost_ptr=None, lx_ptr=None, lxx_ptr=None):
        """Device pointers (or None); asynchronous on the context's stream."""
        self.ctx.check(self.L.ilqr_problem_obstacle_terms_dev(self.h, cost_ptr or None, lx_ptr or None, lxx_ptr or None))

    def close(self):
        if self.h:
            if self.ctx.h:  # a destroyed context has already destroyed its problems
                self.L.ilqr_problem_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _lqt_prototypes(L):
    """The ilqr_lqt_* prototypes, declared on first use (the sanitizer harness's host build of the library has no LQT translation unit)."""
    if getattr(L, "_lqt_declared", False):
        return
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    L.ilqr_lqt_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.c_double, dp, C.c_int, C.POINTER(vp)]
    L.ilqr_lqt_destroy.argtypes = [vp]
    L.ilqr_lqt_destroy.restype = None
    for n in ("set_targets", "set_targets_dev", "get_U", "get_U_dev", "get_X", "get_X_dev", "get_P", "get_d"):
        getattr(L, "ilqr_lqt_" + n).argtypes = [vp, vp]
    L.ilqr_lqt_solve_dp.argtypes = [vp]
    L.ilqr_lqt_solve_lin_al.argtypes = [vp]
    for n in ("ilqr_lqt_command", "ilqr_lqt_command_dev"):
        getattr(L, n).argtypes = [vp, C.c_int, vp, vp]
    L._lqt_declared = True


class LQTBatch:
    """B instances of solver::LQT (ilqr_lqt_*) sharing A, B and R = r I.  Qs: [N][n][n] shared, or [B][N][n][n] with qs_per_instance;
    Qs[N-1] is the terminal weight.  mu: [B][N][n] targets.  r is the R diagonal value (PyLQR's LQT passes pow(float(rfactor), nb_deriv))."""

    def __init__(self, ctx: Context, A, B, Qs, mu, r, qs_per_instance=False):
        A, Bm, Qs, mu = _f64(A), _f64(B), _f64(Qs), _f64(mu)
        if A.ndim != 2 or Bm.ndim != 2 or mu.ndim != 3 or Qs.ndim != (4 if qs_per_instance else 3):
            raise ValueError("LQTBatch: A [n][n], B [n][m], Qs [N][n][n] (or [B][N][n][n] per instance), mu [B][N][n]")
        self.ctx, self.L = ctx, ctx.L
        _lqt_prototypes(self.L)
        self.B, self.N, self.n = mu.shape
        self.m = Bm.shape[1]
        self.per_instance = bool(qs_per_instance)
        self.h = C.c_void_p()
        ctx.check(self.L.ilqr_lqt_create(ctx.h, A.shape[1], self.m, self.N, self.B, _dp(A), _dp(Bm), float(r), _dp(Qs), int(self.per_instance),
                                         C.byref(self.h)))
        ctx._problems.add(self)
        self.set_targets(mu)

    def set_targets(self, mu):
        mu = _f64(mu, (self.B, self.N, self.n))
        self.ctx.check(self.L.ilqr_lqt_set_targets(self.h, mu.ctypes.data))

    def set_targets_dev(self, ptr):
        self.ctx.check(self.L.ilqr_lqt_set_targets_dev(self.h, ptr))

    def solve_dp(self):
        self.ctx.check(self.L.ilqr_lqt_solve_dp(self.h))

    def solve_lin_al(self):
        self.ctx.check(self.L.ilqr_lqt_solve_lin_al(self.h))

    def command(self, t: int, x):
        """The reference's getCommand(t, x) for every instance: x [B][n] -> u [B][m]."""
        x = _f64(x, (self.B, self.n))
        u = np.empty((self.B, self.m))
        self.ctx.check(self.L.ilqr_lqt_command(self.h, int(t), x.ctypes.data, u.ctypes.data))
        return u

    def command_dev(self, t: int, x_ptr, u_ptr):
        self.ctx.check(self.L.ilqr_lqt_command_dev(self.h, int(t), x_ptr, u_ptr))

    def _get(self, name, shape):
        o = np.zeros(shape)
        self.ctx.check(getattr(self.L, "ilqr_lqt_get_" + name)(self.h, o.ctypes.data))
        return o

    def U(self):
        return self._get("U", (self.B, self.N - 1, self.m))

    def X(self):
        return self._get("X", (self.B, self.N, self.n))

    def P(self):
        return self._get("P", ((self.B,) if self.per_instance else ()) + (self.N, self.n, self.n))

    def d(self):
        return self._get("d", (self.B, self.N, self.n))

    def U_dev(self, ptr):
        self.ctx.check(self.L.ilqr_lqt_get_U_dev(self.h, ptr))

    def X_dev(self, ptr):
        self.ctx.check(self.L.ilqr_lqt_get_X_dev(self.h, ptr))

    def close(self):
        if self.h:
            if self.ctx.h:  # a destroyed context has already destroyed its handles
                self.L.ilqr_lqt_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
