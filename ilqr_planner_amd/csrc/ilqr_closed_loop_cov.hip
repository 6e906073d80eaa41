// ilqr_closed_loop_cov.hip -- row kernel of the analytic closed-loop covariance (ilqr_problem_closed_loop_cov) for gfx950 (MI355X), fp64.
//
// The generic kernel (k_cl_cov, ilqr_kernels.hip) gives an instance one lane and keeps its matrices in global memory: a chain of T dependent
// steps of ~2 n_u n_x^2 memory operations each.  Here 16 lanes = one DPP row own an instance (4 instances per wave, the mapping of
// k_backward_rows): lane r < n_x holds ROW r of Sigma in registers and everything of the step that belongs to state r --
//   its own gain row K[i(r)] (loaded by position lane i and shifted 7 lanes up for velocity lane 7 + i; the time lane loads the time control's),
//   xbar_k[r], ubar_k[i(r)], its coefficient b_r and its entry c_r of the time column of B (ilqr_closed_loop_cov.hpp).
// The step is the factorised form of that header, every product a "row += own scalar * broadcast(row of lane j)" with the broadcast a DPP
// row_newbcast operand:
//   G[i(r)] = K[i(r)] Sigma            n_x^2 FMAs per lane: own K[i(r)][j] times row j of Sigma from lane j         (u_var = G . K in the lane)
//   M[r]    = Sigma[r] (+ dt Sigma[7 + r]: a 7-lane row shift) + b_r G[i(r)] + c_r G[last]   (G[last] broadcast from the time lane)
//   H[r][i] = M[r] . K[i]              n_u n_x FMAs per lane: own M[r][j] times K[i][j] from the lane of control i
//   Sigma'[r][c] = M[r][c] (+ dt M[r][7 + c]) + b_c H[r][i(c)] + c_c H[r][last] (+ sigma_w[r]^2 at c = r)           (c_c broadcast from lane c)
// No LDS, nothing couples the waves.  The largest product, G, is written as v_fmac_f64_dpp statements (cv_fmac, the form of k_backward_rows);
// the others use the compiler-visible DPP moves of ilqr_lanes.hpp, which this compiler does not fold into their FMAs (two v_mov_b32_dpp
// and an FMA each).  The record of step k + 1 -- gain row, xbar, ubar -- is loaded before step k computes.
// A lane computes its whole row, so Sigma[r][c] and Sigma[c][r] may differ in the last bits inside the recursion; what is STORED is the lower
// triangle of every lane's row, written to both (r, c) and (c, r): every stored Sigma_k is exactly symmetric.  lim_z is reduced over the
// row's lanes at the end (a minimum: exact in any order).  Layouts of 7-joint problems only; narrower chains take the generic kernel.
// The sums run in another order than the generic kernel's: the two agree to rounding, not bit for bit.
#include <type_traits>

#include "ilqr_closed_loop_cov.hpp"
#include "ilqr_lanes.hpp"
#include "ilqr_step.hpp"

namespace ilqr {

namespace {

// f(integral_constant<int, I>) for I = I0 .. N - 1: a loop whose index is a template argument (the lane of a DPP broadcast)
template <int I, int N, class F>
__device__ __forceinline__ void cv_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        cv_for<I + 1, N>(f);
    }
}

// minimum over the 16 lanes of the DPP row, result in all sixteen (every lane has a source in each of the four moves)
__device__ __forceinline__ double cv_row_min(double v) {
    v = fmin(v, dppz_f64<0xB1>(v));   // quad_perm [1,0,3,2]
    v = fmin(v, dppz_f64<0x4E>(v));   // quad_perm [2,3,0,1]
    v = fmin(v, dppz_f64<0x141>(v));  // row_half_mirror
    v = fmin(v, dppz_f64<0x140>(v));  // row_mirror
    return v;
}

// sum over the 16 lanes of the DPP row, result in all sixteen: cv_row_min's four moves
__device__ __forceinline__ double cv_row_sum(double v) {
    v += dppz_f64<0xB1>(v);
    v += dppz_f64<0x4E>(v);
    v += dppz_f64<0x141>(v);
    v += dppz_f64<0x140>(v);
    return v;
}

#define CV_ALL_ " row_mask:0xf bank_mask:0xf"
// acc[c] += bcast_L(src[c]) * mul for N consecutive columns (N = 8 or 7): the row_newbcast FMA form of k_backward_rows (rw_fmac,
// ilqr_kernels_rowsweep.hip) -- one statement, first the two wait states a DPP read needs after a VALU write of any of its operands; inside
// it no instruction reads what another one wrote
template <int L, int N>
__device__ __forceinline__ void cv_fmac(double* acc, const double* src, double mul) {
    static_assert(N == 8 || N == 7, "columns of a statement");
#define F_(I) "v_fmac_f64_dpp %[a" #I "], %[s" #I "], %[m] row_newbcast:%[L]" CV_ALL_ "\n\t"
    if constexpr (N == 8)
        asm volatile("s_nop 1\n\t" F_(0) F_(1) F_(2) F_(3) F_(4) F_(5) F_(6) F_(7) ""
                     : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), [a3] "+v"(acc[3]), [a4] "+v"(acc[4]), [a5] "+v"(acc[5]), [a6] "+v"(acc[6]), [a7] "+v"(acc[7])
                     : [s0] "v"(src[0]), [s1] "v"(src[1]), [s2] "v"(src[2]), [s3] "v"(src[3]), [s4] "v"(src[4]), [s5] "v"(src[5]), [s6] "v"(src[6]), [s7] "v"(src[7]), [m] "v"(mul),
                       [L] "n"(L));
    else
        asm volatile("s_nop 1\n\t" F_(0) F_(1) F_(2) F_(3) F_(4) F_(5) F_(6) ""
                     : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), [a3] "+v"(acc[3]), [a4] "+v"(acc[4]), [a5] "+v"(acc[5]), [a6] "+v"(acc[6])
                     : [s0] "v"(src[0]), [s1] "v"(src[1]), [s2] "v"(src[2]), [s3] "v"(src[3]), [s4] "v"(src[4]), [s5] "v"(src[5]), [s6] "v"(src[6]), [m] "v"(mul), [L] "n"(L));
#undef F_
}
#undef CV_ALL_

}  // namespace

// CON: the constraint rows are read off Sigma_k as well (ilqr_problem_closed_loop_cov_con).  A template argument: the vector c costs the kernel
// 24 to 66 registers, which the plain covariance call does not pay.
template <class S, bool SYM, bool CON>
__global__ __launch_bounds__(64) void k_cl_cov_rows(Bufs a, ClCovArgs c) {
    constexpr int NX = S::NX, NU = S::NU, ND = S::ND, TM = S::TM, IPW = 4;
    constexpr int ROWP = kd_rowp(NX), RS = SYM ? KD_SYM_RS : NU * ROWP;
    constexpr int TL = NX - 1;   // lane of the time state and the time control (time systems)
    static_assert(NX <= 15 && (!SYM || NX == DOF), "a row per lane of a DPP row; the packed record exists for n_x = 7");
    static_assert(NX == 7 || NX == 8 || NX == 14 || NX == 15, "column groups of cv_fmac");
    static_assert(RS % 2 == 0 && ROWP % 2 == 0, "16-byte loads of a gain row");
    const DevDesc& d = *a.desc;
    const int lane = threadIdx.x, g = lane >> 4, l = lane & 15;
    const int b = blockIdx.x * IPW + g;
    const int Bp = d.Bp, T = d.T, B = d.B;
    const bool ok = b < B;
    const int bb = ok ? b : B - 1;   // lanes of the padding run along on the last instance and store nothing
    const bool isX = l < NX;
    const bool isQ = l < DOF, isV = ND == 2 && l >= DOF && l < 2 * DOF, isT = TM && l == TL;
    const int vx = isX ? l : 0;                                     // this lane's state entry (clamped for the idle lanes)
    const int ci = isT ? NU - 1 : (isQ ? l : (isV ? l - DOF : 0));  // ... and its control row
    const bool isC = isQ || isT;                                    // the lane that loads and reports control ci (a velocity lane takes row ci by a shift)
    const int cur = a.cur[bb];
    const double* pX = a.X[cur] + (size_t)vx * Bp + bb;
    const double* pV = a.X[cur] + (size_t)((ND == 2 && isQ) ? DOF + l : vx) * Bp + bb;   // the velocity of a position lane (time column, 2nd order)
    const double* pU = a.U[cur] + (size_t)ci * Bp + bb;
    const double* pK = a.KD + (size_t)bb * RS + (SYM ? 0 : ci * ROWP);
    const size_t sK = (size_t)Bp * RS, sX = (size_t)NX * Bp, sU = (size_t)NU * Bp;
    int so[SYM ? NX : 1];   // packed record: where entry (ci, j) lies
    if constexpr (SYM) { UNR for (int j = 0; j < NX; j++) so[j] = kd_sym_off(ci, j); }

    // limits of this lane's state entry, both sets
    const bool l1 = isX && d.limits_set && d.lw[vx] != 0, l2 = isX && d.lim2 && d.lw2[vx] != 0;
    const double mx1 = d.smax[vx], mn1 = d.smin[vx], mx2 = d.smax2[vx], mn2 = d.smin2[vx];
    const double sw2 = isX ? c.sw2[vx] : 0.0;

    // The record of a step, every entry read by one lane of the instance: gain row i and ubar_i by the position lane i (the time control's by
    // the time lane), the velocity of the time column by the position lanes of a 2nd-order time system.  The velocity lanes take row i and
    // ubar_i from lane i by a 7-lane shift where the step uses them (row_of); the idle lanes load nothing and hold 0.
    const bool ldK = isC, ldV = TM && ND == 2 && isQ;
    auto load = [&](int k, double (&K_)[NX], double& ub_, double& vb_) {
        UNR for (int j = 0; j < NX; j++) K_[j] = 0.0;
        ub_ = 0.0;
        vb_ = 0.0;
        if (ldK) {
            const double* rec = pK + (size_t)k * sK;
            if constexpr (SYM) {
                UNR for (int j = 0; j < NX; j++) K_[j] = rec[so[j]];
            } else {
                UNR for (int q = 0; q < (NX + 1) / 2; q++) {
                    const double2 v2 = reinterpret_cast<const double2*>(rec)[q];
                    K_[2 * q] = v2.x;
                    if (2 * q + 1 < NX) K_[2 * q + 1] = v2.y;
                }
            }
            ub_ = pU[(size_t)k * sU];
        }
        if (ldV) vb_ = pV[(size_t)k * sX];
    };
    // v of this lane's control row: its own in the lanes that loaded it, lane l - 7's in the velocity lanes (every lane executes the move)
    auto row_of = [&](double v) {
        if constexpr (ND == 2) {
            const double sh = dppz_shr7(v);
            return isV ? sh : v;
        } else {
            return v;
        }
    };
    // the lower triangle of this lane's row to (r, c) and (c, r) of o[NX][NX]
    auto store_sigma = [&](double* o, const double (&S_)[NX]) {
        UNR for (int cc = 0; cc < NX; cc++) {
            if (ok && isX && cc <= l) {
                o[l * NX + cc] = S_[cc];
                o[cc * NX + l] = S_[cc];
            }
        }
    };

    double Sg[NX], kr[NX], ub = 0, vb = 0, xb = isX ? pX[0] : 0.0;
    UNR for (int j = 0; j < NX; j++) kr[j] = 0.0;
    UNR for (int cc = 0; cc < NX; cc++) Sg[cc] = (isX && cc == l) ? c.sx02[vx] : 0.0;
    if (T >= 2) load(0, kr, ub, vb);
    double zmin = INFINITY, zcon = INFINITY;
    int st = 0;  // step table walk
    const int n_kp = d.steps.kp[d.steps.n];
    for (int k = 0; k < T; k++) {
        // ---- what is read off Sigma_k
        if (c.Sigma) store_sigma(c.Sigma + ((size_t)b * T + k) * NX * NX, Sg);
        if (st < d.steps.n && d.steps.t[st] == k) {  // uniform
            if (c.kp_Sigma)
                for (int kpi = d.steps.kp[st]; kpi < d.steps.kp[st + 1]; kpi++) store_sigma(c.kp_Sigma + ((size_t)b * n_kp + kpi) * NX * NX, Sg);
            st++;
        }
        {
            double sii = 0;
            UNR for (int cc = 0; cc < NX; cc++) sii = (cc == l) ? Sg[cc] : sii;
            if (sii > 0) {
                const double sd = sqrt(sii);
                if (l1) zmin = fmin(zmin, fmin(mx1 - xb, xb - mn1) / sd);
                if (l2) zmin = fmin(zmin, fmin(mx2 - xb, xb - mn2) / sd);
            }
        }
        if (k == T - 1) break;
        // ---- the record of the next step, before this one computes (the last step reads its own again)
        double nkr[NX], nub, nvb;
        load(k + 1 < T - 1 ? k + 1 : T - 2, nkr, nub, nvb);
        const double nxb = isX ? pX[(size_t)(k + 1) * sX] : 0.0;
        // ---- the step
        double K_[NX];
        UNR for (int j = 0; j < NX; j++) K_[j] = row_of(kr[j]);
        const double ui = row_of(ub);
        const double dts = TM ? dppz_bcast<TL>(ub) : 0.0;
        const double dt = TM ? dts * dts : d.dt;
        const double b1 = (ND == 1) ? dt : dt * dt / 2;
        const double br = isQ ? b1 : (isV ? dt : 0.0);
        const double cr = TM ? cov_time_col<ND>(isQ, isV, isT, dts, ui, vb) : 0.0;
        const double dtq = (ND == 2 && isQ) ? dt : 0.0;
        if constexpr (CON) {  // the constraint rows of the step
            _Pragma("unroll 1") for (int r = 0; r < a.m; r++) {
                const size_t row = (size_t)(a.per_step ? k : 0) * a.m + r;
                const double* Ar = a.conA + row * (NX + NU);
                // every lane forms c = a_x + K' a_u: K[i][j] from the lane of control i, as in the H block
                double cv[NX];
                UNR for (int j = 0; j < NX; j++) cv[j] = Ar[j];
                cv_for<0, NU>([&](auto ic) {
                    constexpr int I = decltype(ic)::value, L = (I < DOF) ? I : TL;
                    const double au = Ar[NX + I];
                    UNR for (int j = 0; j < NX; j++) cv[j] = fma(dppz_bcast<L>(K_[j]), au, cv[j]);
                });
                // lane l: c[l] (Sigma[l] . c); the idle lanes hold a zero row.  The plan's share of the row: a_x[l] xbar[l] + a_u[i] ubar[i]
                double sc = 0, cl = 0;
                UNR for (int j = 0; j < NX; j++) { sc = fma(Sg[j], cv[j], sc); cl = (j == l) ? cv[j] : cl; }
                const double var = cv_row_sum(cl * sc);
                double mu = isX ? Ar[vx] * xb : 0.0;
                if (isC) mu = fma(Ar[NX + ci], ub, mu);
                mu = cv_row_sum(mu);
                if (c.con_var && ok && l == 0) c.con_var[((size_t)b * (T - 1) + k) * a.m + r] = var;
                if (var > 0) zcon = fmin(zcon, (a.conb[row] - mu) / sqrt(var));
            }
        }
        double G[NX], M[NX], H[NU];
        UNR for (int cc = 0; cc < NX; cc++) G[cc] = 0;
        cv_for<0, NX>([&](auto jc) {
            constexpr int J = decltype(jc)::value;
            constexpr int N0 = (NX == 7 || NX == 14) ? 7 : 8;   // n_x = 7, 8, 14 = 7 + 7, 15 = 8 + 7 columns
            cv_fmac<J, N0>(G, Sg, K_[J]);
            if constexpr (NX > 8) cv_fmac<J, 7>(G + N0, Sg + N0, K_[J]);
        });
        if (c.u_var) {  // uniform
            double s = 0;
            UNR for (int cc = 0; cc < NX; cc++) s = fma(G[cc], K_[cc], s);
            if (ok && isC) c.u_var[((size_t)b * (T - 1) + k) * NU + ci] = s;
        }
        UNR for (int cc = 0; cc < NX; cc++) {
            double m = Sg[cc];
            if (ND == 2) m = fma(dtq, dppz_shl7(Sg[cc]), m);   // row 7 + r of Sigma, in the position lanes
            m = fma(br, G[cc], m);
            if (TM) m = fma(cr, dppz_bcast<TL>(G[cc]), m);
            M[cc] = m;
        }
        cv_for<0, NU>([&](auto ic) {
            constexpr int I = decltype(ic)::value, L = (I < DOF) ? I : TL;   // the lane that holds control row I
            double s = 0;
            UNR for (int j = 0; j < NX; j++) s = fma(M[j], dppz_bcast<L>(K_[j]), s);
            H[I] = s;
        });
        cv_for<0, NX>([&](auto cc_) {
            constexpr int CC = decltype(cc_)::value;
            constexpr bool colQ = CC < DOF, colT = TM && CC == NX - 1;
            constexpr int ctl = colQ ? CC : ((ND == 2 && CC < 2 * DOF) ? CC - DOF : NU - 1);
            double v = M[CC];
            if constexpr (ND == 2 && colQ) v = fma(dt, M[DOF + CC], v);
            if constexpr (!colT) v = fma(colQ ? b1 : dt, H[ctl], v);
            if constexpr (TM != 0) v = fma(dppz_bcast<CC>(cr), H[NU - 1], v);
            Sg[CC] = (CC == l) ? v + sw2 : v;
        });
        UNR for (int j = 0; j < NX; j++) kr[j] = nkr[j];
        ub = nub; vb = nvb; xb = nxb;
    }
    zmin = cv_row_min(zmin);
    if (c.lim_z && ok && l == 0) c.lim_z[b] = zmin;
    if (CON && c.con_z && ok && l == 0) c.con_z[b] = zcon;   // every lane of the row holds the same zcon: the sums above are row sums
}

template <class S, bool SYM>
static void launch_rows(const Bufs& a, const ClCovArgs& c, int B, hipStream_t st) {
    if (c.con_var || c.con_z) hipLaunchKernelGGL((k_cl_cov_rows<S, SYM, true>), dim3((B + 3) / 4), dim3(64), 0, st, a, c);
    else hipLaunchKernelGGL((k_cl_cov_rows<S, SYM, false>), dim3((B + 3) / 4), dim3(64), 0, st, a, c);
}

void launch_closed_loop_cov_rows(int kind, int nd, const Bufs& a, const ClCovArgs& c, int B, hipStream_t st) {
    SysAll::dispatch(kind, nd, [&](auto s) {
        using S = decltype(s);
        if constexpr (S::NX == DOF) {  // the packed symmetric gain record exists for the single-integrator systems only
            if (a.kd_sym) return launch_rows<S, true>(a, c, B, st);
        }
        launch_rows<S, false>(a, c, B, st);
    });
}

}  // namespace ilqr
