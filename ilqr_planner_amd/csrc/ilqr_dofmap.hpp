// ilqr_dofmap.hpp -- where the entries of a chain of 1..7 joints live on the device, which is built for 7 (HIP-free: the map is
// checked on the host by tests/cpp/dofmap_table_main.cpp).
//
// A problem whose chain has dof < 7 moving joints is solved as a 7-joint problem: the lowering appends 7 - dof inert joints (identity
// pre-transform, zero offset, zero axis) behind the last real joint, and every per-joint array is widened through this map.  Joint i < dof
// keeps its index; the velocity dof + i of a 2nd-order state goes to 7 + i; the time entry (state and control) moves to the end.  Device
// entries that no user index reaches are padding: zero state, zero control, zero limit weight and precision, the first joint's control
// weight.  With u = 0 on the padding the inert joints stay at q = 0, where fk's Rodrigues step with a zero axis is the identity exactly
// (sincos(0) = (0, 1)) and their Jacobian columns are zero, so the real entries of every result carry the bits of the narrow problem.
#pragma once

namespace ilqr {

constexpr int DEV_DOF = 7;    // joints every kernel is built for (ilqr_device.hpp: DOF)
constexpr int MAP_MAX = 16;   // entries of one per-step vector (ILQR_MAX_NX + 1)

// One per-step vector (a state, a control, a keypoint target): user index i <-> device index dev[i]; usr[j] = user index of device
// entry j, or -1 for padding.  Passed by value to the layout kernels of ilqr_kernels.hip.
struct IndexMap {
    int n_user, n_dev;
    int dev[MAP_MAX];
    int usr[MAP_MAX];
};

struct DofMap {
    int dof;       // the user's moving joints
    IndexMap x;    // state
    IndexMap u;    // control
    bool identity() const { return dof == DEV_DOF; }
};

// usr[] from dev[] (user entries with dev[i] < 0 are read by nothing)
inline void index_map_fill_usr(IndexMap& m) {
    for (int j = 0; j < MAP_MAX; j++) m.usr[j] = -1;
    for (int i = 0; i < m.n_user; i++)
        if (m.dev[i] >= 0) m.usr[m.dev[i]] = i;
}

// kind: ILQR_SYS_* (0 POS_ORN, 1 POS_ORN_TIME, 2 JOINT, 3 JOINT_TIME); nd: derivatives in the state (1 or 2).  Returns false for
// dof outside 1..7 or an unknown kind / nd.
inline bool dof_map(int kind, int nd, int dof, DofMap& m) {
    if (dof < 1 || dof > DEV_DOF || kind < 0 || kind > 3 || nd < 1 || nd > 2) return false;
    const int tm = (kind == 1 || kind == 3) ? 1 : 0;
    m.dof = dof;
    m.x.n_user = nd * dof + tm;
    m.x.n_dev = nd * DEV_DOF + tm;
    m.u.n_user = dof + tm;
    m.u.n_dev = DEV_DOF + tm;
    for (int j = 0; j < MAP_MAX; j++) m.x.dev[j] = m.u.dev[j] = -1;
    for (int i = 0; i < dof; i++) {
        m.x.dev[i] = i;
        if (nd == 2) m.x.dev[dof + i] = DEV_DOF + i;
        m.u.dev[i] = i;
    }
    if (tm) {
        m.x.dev[nd * dof] = nd * DEV_DOF;
        m.u.dev[dof] = DEV_DOF;
    }
    index_map_fill_usr(m.x);
    index_map_fill_usr(m.u);
    return true;
}

// Target map of a kp_joint keypoint of a PosOrn(Time) system: its n_f = n_x(device) target slots hold the joint vector (+ time) in their
// first n_x entries, on both sides.  User slots behind the user's n_x are read by nothing.  (The targets of a joint-space system are
// states: the state map.)
inline IndexMap joint_target_map(const DofMap& m, int nf) {
    IndexMap t;
    t.n_user = nf;
    t.n_dev = nf;
    for (int j = 0; j < MAP_MAX; j++) t.dev[j] = -1;
    for (int i = 0; i < m.x.n_user && i < nf; i++) t.dev[i] = m.x.dev[i];
    index_map_fill_usr(t);
    return t;
}

}  // namespace ilqr
