// ilqr_batchwide.hpp -- what the two translation units of the wide-basis batch solvers share: ilqr_batchwide.hip (host side, the kernels
// for m = n_kp n_x <= 32) and ilqr_batchwide_big.hip (the kernels for 32 < m <= ILQR_MAX_KP n_x).
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

// M = I + C G | rhs = (r - c) + beta C v0 into the LDS system of instance b, and c into cs, with NT threads (thread tid).  Ends behind a barrier.
template <class S, int MC, int NT>
ILQR_DEV void wl_assemble(const DevDesc& d, const WArgs& c, int b, double beta, int tid, double (*Ms)[MC + 2], double* cs) {
    constexpr int NX = S::NX;
    const int Bp = d.Bp, m = c.m;
    for (int e = tid; e < m * (m + 1); e += NT) {
        const int row = e / (m + 1), col = e % (m + 1), kpi = row / NX, i = row % NX;
        const double* Ck = c.Ckp + (size_t)kpi * NX * NX * Bp;
        double s;
        if (col == m) {
            double cv0 = 0;
            UNR for (int j = 0; j < NX; j++) cv0 += AT(Ck, i * NX + j, b) * AT(c.v0, kpi * NX + j, b);
            s = (AT(c.rkp, row, b) - AT(c.cv, row, b)) + beta * cv0;
        } else {
            s = (row == col) ? 1.0 : 0.0;
            UNR for (int j = 0; j < NX; j++) s += AT(Ck, i * NX + j, b) * c.G[(size_t)(kpi * NX + j) * m + col];
        }
        Ms[row][col] = s;
    }
    if (tid < m) cs[tid] = AT(c.cv, tid, b);
    __syncthreads();
}

// thread tid < m: row tid of ZPZ d, G d, G c (d = xs) into t1, t2, t3, and d out
ILQR_DEV void wl_rows(const WArgs& c, int Bp, int b, int tid, const double* xs, const double* cs, double* t1, double* t2, double* t3) {
    const int m = c.m;
    if (tid < m) {
        double sz = 0, sgd = 0, sgc = 0;
        for (int j = 0; j < m; j++) {
            sz += c.ZPZ[(size_t)tid * m + j] * xs[j];
            sgd += c.G[(size_t)tid * m + j] * xs[j];
            sgc += c.G[(size_t)tid * m + j] * cs[j];
        }
        t1[tid] = sz; t2[tid] = sgd; t3[tid] = sgc;
        AT(c.dvb, tid, b) = xs[tid];
    }
}

// Solves Ms x = Ms[:, m] in place (m x (m+1), m <= 32) with one wave: lane q owns column q during the partial-pivot elimination
// (column m = right-hand side), lane 0 substitutes back; x goes to xs.  Ends behind a barrier.
template <int MC>
ILQR_DEV void wl_lu_solve(double (*Ms)[MC + 2], int m, double* xs, int* prS) {
    const int lane = threadIdx.x;
    for (int k = 0; k < m; k++) {
        if (lane == 0) {
            int pr = k;
            double pv = fabs(Ms[k][k]);
            for (int i = k + 1; i < m; i++) {
                const double v = fabs(Ms[i][k]);
                if (v > pv) { pv = v; pr = i; }
            }
            *prS = pr;
        }
        __syncthreads();
        const int pr = *prS;
        if (lane <= m && lane >= k && pr != k) { const double t0 = Ms[k][lane]; Ms[k][lane] = Ms[pr][lane]; Ms[pr][lane] = t0; }
        __syncthreads();
        if (lane <= m && lane > k) {
            const double piv = Ms[k][k], mk = Ms[k][lane];
            for (int i = k + 1; i < m; i++) Ms[i][lane] -= (Ms[i][k] / piv) * mk;
        }
        __syncthreads();
    }
    if (lane == 0) {
        for (int i = m - 1; i >= 0; i--) {
            double s = Ms[i][m];
            for (int q = i + 1; q < m; q++) s -= Ms[i][q] * xs[q];
            xs[i] = s / Ms[i][i];
        }
    }
    __syncthreads();
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
