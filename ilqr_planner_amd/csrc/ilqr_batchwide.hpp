// ilqr_batchwide.hpp -- what the two translation units of the wide-basis batch solvers share: ilqr_batchwide.hip (tables, host loop,
// the kernels for m = n_kp n_x <= 32) and ilqr_batchwide_big.hip (the kernels for 32 < m <= ILQR_MAX_KP n_x).
#pragma once
#include "ilqr_batch_dev.hpp"

namespace ilqr {

struct WArgs {
    const double *G, *Et, *ZPZ, *PZ;  // shared tables (LTI)
    double *xbk, *av, *v0, *p0, *scal, *cv, *beta, *Ckp, *rkp, *dvb, *sc;
    const double* u0hat;
    int m, it, early_stop;
};

// extra state of the m > 32 kernels (LTI systems): the keypoint states are affine in the step size, x_k(alpha) = xs_k + alpha dxs_k
struct WBig {
    double* xs;   // [n_kp][2][NX][Bp]  x_t, x_{t-1} at the keypoint steps of the current iterate
    double* dxs;  // [n_kp][2][NX][Bp]  their change per unit step: Et d - beta (Wt y0)
    double* kc;   // [n_kp][2][Bp]      task and limit cost of each keypoint at the start (cost0 of the first iteration)
};

struct WTArgs {
    double *Ckp, *rkp, *dun2;
    int m, it, early_stop;
};

// s <- A s + B u of the constant-dt systems
template <class S>
ILQR_DEV void lin_step(const DevDesc& d, double* s, const double* u) {
    const double dt = d.dt, hdt2 = dt * dt / 2;
    if (S::ND == 1) {
        UNR for (int i = 0; i < DOF; i++) s[i] += dt * u[i];
    } else {
        UNR for (int i = 0; i < DOF; i++) {
            s[i] += dt * s[DOF + i] + hdt2 * u[i];
            s[DOF + i] += dt * u[i];
        }
    }
}

// control cost of the family member (beta (1 - al), c + al d):  u'Ru = c00 + (bn^2 - 1) gamma + 2 bn v0.(c + al d) + (c + al d)'G(c + al d)
ILQR_DEV double wl_uru(double c00, double gam, double bn, double al, double v0c, double v0d, double cGc, double cGd, double dGd) {
    return c00 + (bn * bn - 1) * gam + 2 * bn * (v0c + al * v0d) + ((cGc + 2 * al * cGd) + al * al * dGd);
}

// entry (r, cc) of B_j, the linearisation of the step x_{j-1}, u_{j-1} -> x_j (PosOrnTimePlannerSys.cpp:149-185; the 2nd-order
// time column uses the velocity AFTER the step)
template <class S>
ILQR_DEV double wt_bj(int r, int cc, const double* up, const double* xj) {
    constexpr int NX = S::NX, NU = S::NU;
    const double dts = up[NU - 1], dt = dts * dts;
    if (r == NX - 1) return cc == NU - 1 ? 2 * dts : 0.0;
    if (S::ND == 1) {
        if (cc == NU - 1) return 2 * dts * up[r];
        return r == cc ? dt : 0.0;
    }
    if (r < DOF) {
        if (cc == NU - 1) return 2 * dts * xj[DOF + r] + 2 * dts * dts * dts * up[r];
        return r == cc ? dt * dt / 2 : 0.0;
    }
    if (cc == NU - 1) return 2 * dts * up[r - DOF];
    return (r - DOF) == cc ? dt : 0.0;
}

// Launchers of ilqr_batchwide_big.hip (m = n_kp n_x > 32).  kind / nd select the system; grid shapes are fixed per stage, never by B alone.
enum WbStage { WB_INIT, WB_LINEARIZE, WB_SOLVE, WB_LINESEARCH, WB_CONTROLS };
bool wb_lti_launch(WbStage stage, int kind, int nd, int B, int T, int nkp, Bufs& a, const WArgs& c, const WBig& g, hipStream_t s);
bool wb_time_solve_launch(int kind, int nd, int B, Bufs& a, const WTArgs& c, hipStream_t s);

}  // namespace ilqr
