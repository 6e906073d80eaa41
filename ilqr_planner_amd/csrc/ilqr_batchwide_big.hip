// ilqr_batchwide_big.hip -- the wide-basis batch solvers (BatchILQR, BatchILQRCP with Kw > 16; ilqr_batchwide.hip) for many keypoint
// rows: 32 < m = n_kp n_x <= ILQR_MAX_KP n_x (up to 112 on the constant-dt systems, 120 on the time systems).  Same maths as the m <= 32
// kernels, which stay as they are; what changes is where the m-sized data lives.
//
// - No m-long register arrays.  The keypoint states are affine in the step size: with bn = (1 - alpha) beta,
//       x_k(alpha) = [xb + (beta - 1) ab + Et c] + alpha [Et d - beta ab] = xs_k + alpha dxs_k,
//   so the solve writes dxs (one dot product of length m per state row) and the line search evaluates a trial in O(n_x) per keypoint.
//   The winner moves xs, c and beta; the next linearisation reads xs.  c and d stay in global SoA buffers.
// - The m x (m+2) system in LDS, 2 MC threads per instance (MC = 64 or 128 by m, 133 KB of LDS at MC = 128: one workgroup per CU).
//   LU with partial pivoting: the pivot by a wave-level max reduction (first row of the largest |.|, as the serial search), the
//   multipliers in one pass, the update with a thread per (column, row parity); back substitution by column sweeps.  The arithmetic of
//   the elimination is that of the m <= 32 kernels (same multipliers, same updates); only the back substitution sums in another order.
// - Time systems: G = sum_j V_j R^-1 V_j' accumulates in registers (thread = one column and one row parity, MC / 2 entries), is stored
//   into the LDS system, and M = I + C G is formed in place over it block row by block row (row block k of M needs row block k of G).
// No kernel here carries a private segment; none is chosen by batch size.
// The assembly of M = I + C G | rhs and the rows of ZPZ d, G d, G c are those of k_wl_solve (ilqr_batchwide.hpp: wl_assemble, wl_rows).
#include "ilqr_batchcp.hpp"

#include <cmath>

#include "ilqr_batch_dev.hpp"
#include "ilqr_batchwide.hpp"

namespace ilqr {

// Solves Ms x = Ms[:, m] in place (m x (m+1) in the first m rows of Ms) with 2 MC threads; x goes to xs.  Ends behind a barrier.
template <int MC>
ILQR_DEV void wb_lu_solve(double (*Ms)[MC + 2], int m, double* xs, int* prS, double* pvS) {
    constexpr int NT = 2 * MC;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int k = 0; k < m; k++) {
        if (tid < 64) {  // pivot: the first row of the largest |Ms[i][k]|, i >= k
            int pr = k;
            double pv = fabs(Ms[k][k]);
            for (int i = k + 1 + lane; i < m; i += 64) {
                const double v = fabs(Ms[i][k]);
                if (v > pv) { pv = v; pr = i; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(pv, o);
                const int oi = __shfl_xor(pr, o);
                if (ov > pv || (ov == pv && oi < pr)) { pv = ov; pr = oi; }
            }
            if (lane == 0) { prS[0] = pr; pvS[0] = Ms[pr][k]; pvS[1] = Ms[k][k]; }
        }
        __syncthreads();
        const int pr = prS[0];
        const double piv = pvS[0], akk = pvS[1];
        // row swap in columns k+1 .. m; column k becomes the multipliers l_i = a_ik / piv (read after the swap)
        if (pr != k)
            for (int q = k + 1 + tid; q <= m; q += NT) { const double t0 = Ms[k][q]; Ms[k][q] = Ms[pr][q]; Ms[pr][q] = t0; }
        for (int i = k + 1 + tid; i < m; i += NT) Ms[i][k] = ((i == pr) ? akk : Ms[i][k]) / piv;
        if (tid == 0) Ms[k][k] = piv;
        __syncthreads();
        {
            const int col = k + 1 + (tid % MC);
            if (col <= m) {
                const double mk = Ms[k][col];
                for (int i = k + 1 + tid / MC; i < m; i += 2) Ms[i][col] -= Ms[i][k] * mk;
            }
        }
        __syncthreads();
    }
    for (int i = m - 1; i >= 0; i--) {  // column sweep: x_i, then the right-hand side of the rows above loses column i
        const double xi = Ms[i][m] / Ms[i][i];
        if (tid == 0) xs[i] = xi;
        if (tid < i) Ms[tid][m] -= Ms[tid][i] * xi;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ LTI systems

// One wave per instance: lanes own columns lane, lane + 64 of p0 = (PSI Z)' u0^; all lanes walk the three rollouts of k_wl_init, lane 0
// records (and starts xs at the rollout of u0: beta = 1, c = 0).
template <class S, int MC>
__global__ __launch_bounds__(64) void k_wb_init(Bufs a, WArgs c, WBig g) {
    constexpr int NX = S::NX, NU = S::NU, NJ = MC / 64;
    const DevDesc& d = *a.desc;
    const int lane = threadIdx.x, b = blockIdx.x;
    const int Bp = d.Bp, T = d.T, m = c.m;
    int jj[NJ];
    double p0[NJ];
    UNR for (int q = 0; q < NJ; q++) { jj[q] = (lane + 64 * q < m) ? lane + 64 * q : 0; p0[q] = 0; }
    double x[NX], xp[NX], xh[NX], xhp[NX], xz[NX], xzp[NX], sv[NX], u[NU], uh[NU], zero[NU], xn[NX];
    UNR for (int i = 0; i < NU; i++) zero[i] = 0;
    init_state<S>(d, a, b, x);
    UNR for (int i = 0; i < NX; i++) { xp[i] = xh[i] = xhp[i] = xz[i] = xzp[i] = x[i]; sv[i] = 0; }
    double c00 = 0, gam = 0, pi = 0;
    int kpi = 0;
    auto record = [&]() {
        if (lane == 0) {
            double* xb = c.xbk + (size_t)kpi * 2 * NX * Bp;
            double* xc = g.xs + (size_t)kpi * 2 * NX * Bp;
            double* ab = c.av + (size_t)kpi * 2 * NX * Bp;
            UNR for (int r = 0; r < NX; r++) {
                AT(xb, r, b) = x[r];
                AT(xb, NX + r, b) = xp[r];
                AT(xc, r, b) = x[r];
                AT(xc, NX + r, b) = xp[r];
                AT(ab, r, b) = xh[r] - xz[r];
                AT(ab, NX + r, b) = xhp[r] - xzp[r];
                AT(c.v0, kpi * NX + r, b) = sv[r];
            }
        }
        kpi++;
    };
    if (kpi < d.n_kp && d.kp_t[kpi] == 0) record();
    for (int s = 0; s < T - 1; s++) {
        UNR for (int i = 0; i < NU; i++) {
            u[i] = AT(a.U0, s * NU + i, b);
            uh[i] = AT(c.u0hat, s * NU + i, b);
            c00 += u[i] * d.R_diag[i] * u[i];
            gam += u[i] * d.R_diag[i] * uh[i];
            pi += uh[i] * uh[i];
            const double* pz = c.PZ + (size_t)(s * NU + i) * m;
            UNR for (int q = 0; q < NJ; q++) p0[q] += pz[jj[q]] * uh[i];
        }
        dyn_step<S>(d, x, u, xn);
        UNR for (int i = 0; i < NX; i++) { xp[i] = x[i]; x[i] = xn[i]; }
        dyn_step<S>(d, xh, uh, xn);
        UNR for (int i = 0; i < NX; i++) { xhp[i] = xh[i]; xh[i] = xn[i]; }
        dyn_step<S>(d, xz, zero, xn);
        UNR for (int i = 0; i < NX; i++) { xzp[i] = xz[i]; xz[i] = xn[i]; }
        if (s >= 1) lin_step<S>(d, sv, uh);  // block 0 of the reference's Su is zero
        if (kpi < d.n_kp && d.kp_t[kpi] == s + 1) record();
    }
    UNR for (int q = 0; q < NJ; q++)
        if (lane + 64 * q < m) { AT(c.p0, lane + 64 * q, b) = p0[q]; AT(c.cv, lane + 64 * q, b) = 0; }
    if (lane != 0) return;
    AT(c.scal, 0, b) = c00;
    AT(c.scal, 1, b) = gam;
    AT(c.scal, 2, b) = pi;
    c.beta[b] = 1.0;
    batch_reset_instance(a, b);
}

// One lane per (instance, keypoint): C_k = J'QJ + L, r_k = J'Q e + L ql at the iterate's keypoint states xs, row by row to memory as
// k_kp_derivs does (the lane never holds the n_x x n_x matrix).  First iteration: the keypoint's task and limit cost into kc.
template <class S>
__global__ __launch_bounds__(64) void k_wb_linearize(Bufs a, WArgs c, WBig g) {
    constexpr int NX = S::NX;
    constexpr int ROLLN = (!S::JOINT && S::ND == 1) ? 64 : 0;
    __shared__ double sj[ROLLN ? 7 * DOF : 1][64];
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x, kpi = blockIdx.y;
    if (b >= d.B || !a.active[b]) return;
    const int Bp = d.Bp;
    const double* xc = g.xs + (size_t)kpi * 2 * NX * Bp;
    double x[NX], xp[NX], Ld[NX], ql[NX];
    UNR for (int r = 0; r < NX; r++) { x[r] = AT(xc, r, b); xp[r] = AT(xc, NX + r, b); }
    if (d.kp_t[kpi] > 0) limit_terms<S>(d, xp, Ld, ql);
    else { UNR for (int r = 0; r < NX; r++) { Ld[r] = 0; ql[r] = 0; } }
    double* Ck = c.Ckp + (size_t)kpi * NX * NX * Bp;
    stage_derivs_rows<S, true, ROLLN, false>(d, a, b, x, kpi, &sj[0][threadIdx.x], [&](int i, const double* row, double lxi) {
        double ldi = 0, qli = 0;
        UNR for (int r = 0; r < NX; r++)
            if (r == i) { ldi = Ld[r]; qli = ql[r]; }
        UNR for (int s = 0; s < NX; s++) AT(Ck, i * NX + s, b) = row[s] + ((s == i) ? ldi : 0.0);
        AT(c.rkp, kpi * NX + i, b) = -lxi + ldi * qli;
    });
    if (c.it != 0) return;
    double tg[S::NF], cl = 0;
    UNR for (int i = 0; i < S::NF; i++) tg[i] = AT(a.kp_tg, kpi * S::NF + i, b);
    UNR for (int r = 0; r < NX; r++) cl += ql[r] * Ld[r] * ql[r];
    AT(g.kc, 2 * kpi, b) = kp_cost<S>(d, kpi, tg, x, nullptr);
    AT(g.kc, 2 * kpi + 1, b) = cl;
}

// (I + C G) d = (r - c) + beta C v0, 2 MC threads per instance.  Leaves d, the scalars of the line search
//   sc = { v0.c, c'Gc, v0.d, c'Gd, d'Gd, ||PSI dw||^2 },  dw = Z d - beta y0
// and dxs = Et d - beta ab; in the first iteration also cost0 from the keypoint terms of k_wb_linearize.
template <class S, int MC>
__global__ __launch_bounds__(2 * MC) void k_wb_solve(Bufs a, WArgs c, WBig g) {
    constexpr int NT = 2 * MC;
    __shared__ double Ms[MC][MC + 2], xs[MC], cs[MC], t1[MC], t2[MC], t3[MC], pvS[2];
    __shared__ int prS[1];
    const DevDesc& d = *a.desc;
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
    if (!a.active[b]) return;  // uniform
    const int Bp = d.Bp, m = c.m, nkp = d.n_kp;
    const double beta = c.beta[b];
    if (c.it == 0 && tid == 0) {  // k_wl_linearize's cost0: (task + limits) + u'Ru at beta = 1, c = 0
        double ce = 0, cl = 0;
        for (int k = 0; k < nkp; k++) { ce += AT(g.kc, 2 * k, b); cl += AT(g.kc, 2 * k + 1, b); }
        a.cost[b] = (ce + cl) + wl_uru(AT(c.scal, 0, b), AT(c.scal, 1, b), beta, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0);
    }
    wl_assemble<S, MC, NT>(d, c, b, beta, tid, Ms, cs);
    wb_lu_solve<MC>(Ms, m, xs, prS, pvS);
    wl_rows(c, Bp, b, tid, xs, cs, t1, t2, t3);
    if (tid < 2 * m) {  // state row tid of the keypoint records: dxs = Et d - beta ab
        const double* et = c.Et + (size_t)tid * m;
        double s = 0;
        for (int j = 0; j < m; j++) s += et[j] * xs[j];
        AT(g.dxs, tid, b) = s - beta * AT(c.av, tid, b);
    }
    __syncthreads();
    if (tid < 64) {
        double dZd = 0, dp0 = 0, v0d = 0, cGd = 0, dGd = 0, v0c = 0, cGc = 0;
        for (int i = lane; i < m; i += 64) {
            const double di = xs[i], ci = cs[i], v0i = AT(c.v0, i, b);
            dZd += di * t1[i];
            dGd += di * t2[i];
            cGd += di * t3[i];
            cGc += ci * t3[i];
            dp0 += di * AT(c.p0, i, b);
            v0d += di * v0i;
            v0c += v0i * ci;
        }
        for (int o = 32; o > 0; o >>= 1) {
            dZd += __shfl_xor(dZd, o); dp0 += __shfl_xor(dp0, o); v0d += __shfl_xor(v0d, o); cGd += __shfl_xor(cGd, o);
            dGd += __shfl_xor(dGd, o); v0c += __shfl_xor(v0c, o); cGc += __shfl_xor(cGc, o);
        }
        if (lane == 0) {
            AT(c.sc, 0, b) = v0c; AT(c.sc, 1, b) = cGc; AT(c.sc, 2, b) = v0d; AT(c.sc, 3, b) = cGd; AT(c.sc, 4, b) = dGd;
            AT(c.sc, 5, b) = dZd - 2 * beta * dp0 + beta * beta * AT(c.scal, 2, b);
        }
    }
}

// Backtracking with all step sizes at once, 16 lanes per instance (k_wl_linesearch): lane l tries alpha = 2^-l on the affine keypoint
// states; the 16 lanes then move c, xs of the winner.
template <class S>
__global__ __launch_bounds__(64) void k_wb_linesearch(Bufs a, WArgs c, WBig g) {
    constexpr int NX = S::NX;
    const DevDesc& d = *a.desc;
    const int lane = threadIdx.x, l = lane & 15, bq = blockIdx.x * 4 + (lane >> 4);
    const bool ok = bq < d.B && a.active[bq < d.B ? bq : 0];
    const int b = ok ? bq : 0;
    const int Bp = d.Bp, m = c.m, nkp = d.n_kp;
    const double beta = c.beta[b], cost0 = a.cost[b];
    const double alpha = ldexp(1.0, -(l < 11 ? l : 10)), bn = (1 - alpha) * beta;
    double cost_e = 0, cost_l = 0;
    for (int kpi = 0; kpi < nkp; kpi++) {
        const double* xc = g.xs + (size_t)kpi * 2 * NX * Bp;
        const double* dx = g.dxs + (size_t)kpi * 2 * NX * Bp;
        double x[NX], xp[NX], tg[S::NF];
        UNR for (int r = 0; r < NX; r++) { x[r] = fma(alpha, AT(dx, r, b), AT(xc, r, b)); xp[r] = fma(alpha, AT(dx, NX + r, b), AT(xc, NX + r, b)); }
        UNR for (int i = 0; i < S::NF; i++) tg[i] = AT(a.kp_tg, kpi * S::NF + i, b);
        cost_e += kp_cost<S>(d, kpi, tg, x, nullptr);
        if (d.kp_t[kpi] > 0) {
            double Ld[NX], ql[NX];
            limit_terms<S>(d, xp, Ld, ql);
            UNR for (int r = 0; r < NX; r++) cost_l += ql[r] * Ld[r] * ql[r];
        }
    }
    const double uru = wl_uru(AT(c.scal, 0, b), AT(c.scal, 1, b), bn, alpha, AT(c.sc, 0, b), AT(c.sc, 2, b), AT(c.sc, 1, b), AT(c.sc, 3, b), AT(c.sc, 4, b));
    const double cost = (cost_e + cost_l) + uru;
    const bool take = (l < 11) && ((cost < cost0) || (alpha < 1e-3));
    const unsigned long long mk = __ballot(take ? 1 : 0);
    const int win = __ffs((unsigned)((mk >> (lane & 48)) & 0xffffull)) - 1;
    if (!ok) return;
    const double aw = ldexp(1.0, -win);
    for (int j = l; j < m; j += 16) AT(c.cv, j, b) = fma(aw, AT(c.dvb, j, b), AT(c.cv, j, b));
    for (int r = l; r < 2 * m; r += 16) AT(g.xs, r, b) = fma(aw, AT(g.dxs, r, b), AT(g.xs, r, b));  // the winner's trial states, same bits
    if (l != win) return;
    c.beta[b] = bn;
    batch_record_winner(a, Bp, b, c.it, alpha, cost0, cost);
    const double dun2 = AT(c.sc, 5, b);
    if (c.early_stop && alpha * sqrt(dun2 > 0 ? dun2 : 0.0) < 1e-3) a.active[b] = 0;  // :167
}

// u = u0 + (beta - 1) u0^ + (PSI Z) c, one lane per (instance, step); c streams from memory
template <class S>
__global__ __launch_bounds__(64) void k_wb_controls(Bufs a, WArgs c) {
    constexpr int NU = S::NU;
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
    if (b >= d.B) return;
    const int Bp = d.Bp, m = c.m;
    double du[NU];
    UNR for (int i = 0; i < NU; i++) du[i] = 0;
    for (int j = 0; j < m; j++) {
        const double cj = AT(c.cv, j, b);
        UNR for (int i = 0; i < NU; i++) du[i] += c.PZ[(size_t)(s * NU + i) * m + j] * cj;
    }
    const double bm1 = c.beta[b] - 1;
    UNR for (int i = 0; i < NU; i++) AT(a.U[0], s * NU + i, b) = (AT(a.U0, s * NU + i, b) + bm1 * AT(c.u0hat, s * NU + i, b)) + du[i];
}

// ------------------------------------------------------------------------------------------------ time systems, identity basis

// k_wt_solve with 2 MC threads per instance: thread = column tid % MC and row parity tid / MC of G (MC / 2 accumulators), the system
// formed in place over G, the LU of wb_lu_solve, then du_j = R^-1 V_j' kappa - u_j with a thread per column block.
template <class S, int MC>
__global__ __launch_bounds__(2 * MC) void k_wtb_solve(Bufs a, WTArgs c) {
    constexpr int NX = S::NX, NU = S::NU, NT = 2 * MC, GE = MC / 2;
    __shared__ double Vj[MC][NU], Ms[MC][MC + 2], vuS[MC], kap[MC], tkS[MAX_KP], dnS[NT / 64], pvS[2];
    __shared__ int prS[1];
    const DevDesc& d = *a.desc;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (!a.active[b]) return;
    const int Bp = d.Bp, T = d.T, m = c.m, nkp = d.n_kp;
    const double* X = a.X[0];
    const double* U = a.U[0];
    double rinv[NU];
    UNR for (int i = 0; i < NU; i++) rinv[i] = 1.0 / d.R_diag[i];
    int jmax = 0;
    for (int k = 0; k < nkp; k++) {
        const int t = d.kp_t[k];
        if (t - 1 > jmax) jmax = t - 1;
    }
    if (tid < nkp) {
        const int t = d.kp_t[tid];
        tkS[tid] = t >= 1 ? AT(X, (t - 1) * NX + NX - 1, b) : 0.0;
    }
    __syncthreads();
    const int gc = tid % MC, rp = tid / MC;
    double gacc[GE], vu = 0;
    UNR for (int i = 0; i < GE; i++) gacc[i] = 0;
    for (int j = 1; j <= jmax && j <= T - 2; j++) {
        double up[NU], uj[NU], xj[NX];
        UNR for (int i = 0; i < NU; i++) { up[i] = AT(U, (j - 1) * NU + i, b); uj[i] = AT(U, j * NU + i, b); }
        UNR for (int i = 0; i < NX; i++) xj[i] = AT(X, j * NX + i, b);
        for (int idx = tid; idx < m * NU; idx += NT) {
            const int row = idx / NU, cc = idx % NU, k = row / NX, r = row % NX;
            double v = 0;
            if (d.kp_t[k] > j) {
                v = wt_bj<S>(r, cc, up, xj);
                if (S::ND == 2 && r < DOF) v += (tkS[k] - xj[NX - 1]) * wt_bj<S>(DOF + r, cc, up, xj);
            }
            Vj[row][cc] = v;
        }
        __syncthreads();
        if (gc < m) {
            double vc[NU];
            UNR for (int cc = 0; cc < NU; cc++) vc[cc] = rinv[cc] * Vj[gc][cc];
            UNR for (int i = 0; i < GE; i++) {
                const int row = rp + 2 * i;
                if (row < m) {
                    double s = 0;
                    UNR for (int cc = 0; cc < NU; cc++) s += Vj[row][cc] * vc[cc];
                    gacc[i] += s;
                }
            }
        }
        if (tid < m) { UNR for (int cc = 0; cc < NU; cc++) vu += Vj[tid][cc] * uj[cc]; }
        __syncthreads();
    }
    if (gc < m) {
        UNR for (int i = 0; i < GE; i++)
            if (rp + 2 * i < m) Ms[rp + 2 * i][gc] = gacc[i];
    }
    if (tid < m) vuS[tid] = vu;
    __syncthreads();
    // M = I + C G | rhs = r + C (V u), in place: task (k, col) reads column col of row block k of G, writes the same entries of M
    for (int e = tid; e < nkp * (m + 1); e += NT) {
        const int k = e / (m + 1), col = e % (m + 1);
        const double* Ck = c.Ckp + (size_t)k * NX * NX * Bp;
        double gv[NX];
        UNR for (int jj = 0; jj < NX; jj++) gv[jj] = (col == m) ? vuS[k * NX + jj] : Ms[k * NX + jj][col];
        UNR for (int i = 0; i < NX; i++) {
            const int row = k * NX + i;
            double s = (col == m) ? AT(c.rkp, row, b) : ((row == col) ? 1.0 : 0.0);
            UNR for (int jj = 0; jj < NX; jj++) s += AT(Ck, i * NX + jj, b) * gv[jj];
            Ms[row][col] = s;
        }
    }
    __syncthreads();
    wb_lu_solve<MC>(Ms, m, kap, prS, pvS);
    double dn = 0;
    for (int j = tid; j <= T - 2; j += NT) {
        double lam[NX], uj[NU], t[NU];
        UNR for (int r = 0; r < NX; r++) lam[r] = 0;
        UNR for (int i = 0; i < NU; i++) { uj[i] = AT(U, j * NU + i, b); t[i] = 0; }
        if (j >= 1 && j <= jmax) {
            double up[NU], xj[NX];
            UNR for (int i = 0; i < NU; i++) up[i] = AT(U, (j - 1) * NU + i, b);
            UNR for (int i = 0; i < NX; i++) xj[i] = AT(X, j * NX + i, b);
            for (int k = 0; k < nkp; k++) {  // lambda = sum_k Phi_{k,j}' kappa_k
                if (d.kp_t[k] <= j) continue;
                const double dl = tkS[k] - xj[NX - 1];
                UNR for (int r = 0; r < NX; r++) lam[r] += kap[k * NX + r];
                if (S::ND == 2) { UNR for (int r = 0; r < DOF; r++) lam[DOF + r] += dl * kap[k * NX + r]; }
            }
            UNR for (int cc = 0; cc < NU; cc++) {  // t = B_j' lambda
                double s = 0;
                UNR for (int r = 0; r < NX; r++) s += wt_bj<S>(r, cc, up, xj) * lam[r];
                t[cc] = s;
            }
        }
        UNR for (int cc = 0; cc < NU; cc++) {
            const double du = t[cc] * rinv[cc] - uj[cc];
            AT(a.U[1], j * NU + cc, b) = du;
            dn += du * du;
        }
    }
    for (int o = 32; o > 0; o >>= 1) dn += __shfl_xor(dn, o);
    if (lane == 0) dnS[tid / 64] = dn;
    __syncthreads();
    if (tid == 0) {
        double s = 0;
        UNR for (int w = 0; w < NT / 64; w++) s += dnS[w];
        c.dun2[b] = s;
    }
}

// ------------------------------------------------------------------------------------------------ launchers

template <class S, int MC>
static void wb_lti_stage(WbStage stage, int B, int T, int nkp, Bufs& a, const WArgs& c, const WBig& g, hipStream_t s) {
    switch (stage) {
    case WB_INIT: hipLaunchKernelGGL((k_wb_init<S, MC>), dim3(B), dim3(64), 0, s, a, c, g); break;
    case WB_LINEARIZE: hipLaunchKernelGGL((k_wb_linearize<S>), dim3((B + 63) / 64, nkp), dim3(64), 0, s, a, c, g); break;
    case WB_SOLVE: hipLaunchKernelGGL((k_wb_solve<S, MC>), dim3(B), dim3(2 * MC), 0, s, a, c, g); break;
    case WB_LINESEARCH: hipLaunchKernelGGL((k_wb_linesearch<S>), dim3((B + 3) / 4), dim3(64), 0, s, a, c, g); break;
    case WB_CONTROLS: hipLaunchKernelGGL((k_wb_controls<S>), dim3((B + 63) / 64, T - 1), dim3(64), 0, s, a, c); break;
    }
}

// MC = 64 where m <= 64, else 128 (only the 2nd-order systems reach it)
template <class S>
static bool wb_lti_m(WbStage stage, int B, int T, int nkp, Bufs& a, const WArgs& c, const WBig& g, hipStream_t s) {
    if (c.m <= 32) return false;
    if (c.m <= 64) { wb_lti_stage<S, 64>(stage, B, T, nkp, a, c, g, s); return true; }
    if constexpr (MAX_KP * S::NX > 64) {
        if (c.m <= 128) { wb_lti_stage<S, 128>(stage, B, T, nkp, a, c, g, s); return true; }
    }
    return false;
}

bool wb_lti_launch(WbStage stage, int kind, int nd, int B, int T, int nkp, Bufs& a, const WArgs& c, const WBig& g, hipStream_t s) {
    bool done = false;
    SysList<Sys<0, 1>, Sys<0, 2>, Sys<2, 1>>::dispatch(kind, nd, [&](auto sys) { done = wb_lti_m<decltype(sys)>(stage, B, T, nkp, a, c, g, s); });
    return done;
}

template <class S>
static bool wtb_m(int B, Bufs& a, const WTArgs& c, hipStream_t s) {
    if (c.m <= 32) return false;
    if (c.m <= 64) { hipLaunchKernelGGL((k_wtb_solve<S, 64>), dim3(B), dim3(128), 0, s, a, c); return true; }
    if constexpr (MAX_KP * S::NX > 64) {
        if (c.m <= 128) { hipLaunchKernelGGL((k_wtb_solve<S, 128>), dim3(B), dim3(256), 0, s, a, c); return true; }
    }
    return false;
}

bool wb_time_solve_launch(int kind, int nd, int B, Bufs& a, const WTArgs& c, hipStream_t s) {
    bool done = false;
    SysList<Sys<1, 1>, Sys<1, 2>, Sys<3, 1>>::dispatch(kind, nd, [&](auto sys) { done = wtb_m<decltype(sys)>(B, a, c, s); });
    return done;
}

}  // namespace ilqr
