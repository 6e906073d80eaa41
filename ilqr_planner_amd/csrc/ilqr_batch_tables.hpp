// ilqr_batch_tables.hpp -- the shared tables of the batch Gauss-Newton solvers on the constant-dt systems (ilqr_batchcp.hip: narrow bases in
// coefficient space; ilqr_batchwide.hip: wide bases and BatchILQR's identity basis), what they were built from (BatchTableSig) and what the
// device buffers are sized from (BatchSizes).  Plain C++17 on plain values, no HIP: checked on the host by tests/cpp/batch_tables_main.cpp.
//
// A constant-dt system has n_x = nd n_u, A = [I dt I; 0 I] (nd = 2) or I (nd = 1) and B = [dt^2/2 I; dt I] or dt I.  With PSI the
// (T-1) n_u x Kw basis (row block i = PSI_i), the tables are, at the keypoint steps t_k:
//   wt    Wt_{t_k} and Wt_{t_k - 1}: the TRUE sensitivity d x_t / d w,  Wt_{i+1} = A Wt_i + B PSI_i from Wt_0 = 0
//   wr    Wr_{t_k}: the reference's shifted one (block j of Su meets B_j = dx_j / du_{j-1}, BatchILQRCP.cpp:61-97, quirk D-1),
//         Wr_{i+1} = A Wr_i + B PSI_i for i >= 1 from Wr_1 = 0.  Stacked over the keypoints it is V = Su PSI (m x Kw, m = n_kp n_x).
//   narrow (Kw <= 16, columns zero-padded to ld = 16):  H0 = PSI'R PSI with 1 on the padded diagonal, pp = PSI'PSI
//   wide:  Z = H0^-1 V' (never kept),  G = V Z (symmetrised),  Et = wt Z,  PZ = PSI Z,  ZPZ = PZ'PZ,  h0inv = H0^-1 (Cholesky)
// The identity basis (psi == nullptr, Kw = (T-1) n_u) never forms a Kw x Kw matrix: H0 = R is diagonal.
// Every sum runs in one fixed order (stated at each loop): the tables are the same bits whoever builds them.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

namespace ilqr {

struct BatchTableIn {
    int nd = 1, n_x = 0, n_u = 0, T = 0;
    double dt = 0;
    int n_kp = 0;
    const int* kp_t = nullptr;        // [n_kp] keypoint steps, ascending
    const double* R_diag = nullptr;   // [n_u]
    const double* psi = nullptr;      // [(T-1) n_u][Kw] row-major, or null: the identity
    int Kw = 0;
    int ld = 0;                       // columns of wt / wr / psip / H0 / pp (>= Kw; the columns past Kw are padding)
    bool sens = true;                 // wt / wr (/ pp) are wanted: false on the general narrow path, which has per-instance sensitivities
    int rows() const { return (T - 1) * n_u; }
};

// What a set of tables was built from.  valid = false: no tables.
struct BatchTableSig {
    bool valid = false, ident = false, sens = false;
    int nd = 0, n_x = 0, n_u = 0, T = 0, n_kp = 0, Kw = 0, ld = 0;
    double dt = 0;
    std::vector<int> kp_t;
    std::vector<double> R_diag, psi;

    bool same(const BatchTableIn& in) const {
        if (!valid || ident != (in.psi == nullptr) || sens != in.sens) return false;
        if (nd != in.nd || n_x != in.n_x || n_u != in.n_u || T != in.T || n_kp != in.n_kp || Kw != in.Kw || ld != in.ld) return false;
        if (!(dt == in.dt)) return false;
        if (!std::equal(kp_t.begin(), kp_t.end(), in.kp_t) || !std::equal(R_diag.begin(), R_diag.end(), in.R_diag)) return false;
        return ident || (psi.size() == (size_t)in.rows() * in.Kw && !std::memcmp(psi.data(), in.psi, sizeof(double) * psi.size()));
    }
    void set(const BatchTableIn& in) {
        valid = true; ident = in.psi == nullptr; sens = in.sens;
        nd = in.nd; n_x = in.n_x; n_u = in.n_u; T = in.T; n_kp = in.n_kp; Kw = in.Kw; ld = in.ld; dt = in.dt;
        kp_t.assign(in.kp_t, in.kp_t + in.n_kp);
        R_diag.assign(in.R_diag, in.R_diag + in.n_u);
        if (ident) psi.clear();
        else psi.assign(in.psi, in.psi + (size_t)in.rows() * in.Kw);
    }
    void clear() { *this = BatchTableSig(); }
};

// What the device buffers of a batch solver state are sized from.
struct BatchSizes {
    enum Layout { NONE, NARROW, WIDE_LTI, WIDE_TIME };
    int layout = NONE;
    int n_x = 0, n_kp = 0, rows = 0, cols = 0, Bp = 0;  // rows = (T-1) n_u; cols = the padded Kw (narrow) or Kw (wide)
    bool ident = false;                                // wide: no PSI, H0^-1 or projection buffers
    bool operator==(const BatchSizes& o) const {
        return layout == o.layout && n_x == o.n_x && n_kp == o.n_kp && rows == o.rows && cols == o.cols && Bp == o.Bp && ident == o.ident;
    }
    bool operator!=(const BatchSizes& o) const { return !(*this == o); }
};

// W <- A W + B PSI_i for an n_x x ld tile W (row-major).  Per entry: the position row takes dt x the OLD velocity row, then the basis term.
inline void sens_advance(const BatchTableIn& in, double* W, int i) {
    const int dof = in.n_u, ld = in.ld, Kw = in.Kw;
    const double dt = in.dt, hdt2 = dt * dt / 2;
    if (in.nd == 2)
        for (int r = 0; r < dof; r++)
            for (int q = 0; q < ld; q++) W[(size_t)r * ld + q] += dt * W[(size_t)(dof + r) * ld + q];
    for (int r = 0; r < dof; r++) {
        if (!in.psi) {
            const int q = i * in.n_u + r;
            if (in.nd == 1) W[(size_t)r * ld + q] += dt;
            else { W[(size_t)r * ld + q] += hdt2; W[(size_t)(dof + r) * ld + q] += dt; }
        } else {
            const double* pr = in.psi + (size_t)(i * in.n_u + r) * Kw;
            for (int q = 0; q < ld; q++) {
                const double ps = q < Kw ? pr[q] : 0.0;
                if (in.nd == 1) W[(size_t)r * ld + q] += dt * ps;
                else { W[(size_t)r * ld + q] += hdt2 * ps; W[(size_t)(dof + r) * ld + q] += dt * ps; }
            }
        }
    }
}

// wt [n_kp][2][n_x][ld] (Wt at the keypoint step, then at the step before it; zero where there is none) and wr [n_kp][n_x][ld]
inline void sens_tables(const BatchTableIn& in, std::vector<double>& wt, std::vector<double>& wr) {
    const size_t tile = (size_t)in.n_x * in.ld, nk = in.n_kp > 0 ? in.n_kp : 1;
    wt.assign(nk * 2 * tile, 0.0);
    wr.assign(nk * tile, 0.0);
    std::vector<double> Wt(tile, 0.0), Wr(tile, 0.0);
    auto sample = [&](int i) {  // Wt = Wt_i, Wr = Wr_i
        for (int t = 0; t < in.n_kp; t++) {
            if (in.kp_t[t] == i) {
                std::copy(Wt.begin(), Wt.end(), wt.begin() + ((size_t)t * 2 + 0) * tile);
                std::copy(Wr.begin(), Wr.end(), wr.begin() + (size_t)t * tile);
            }
            if (in.kp_t[t] - 1 == i) std::copy(Wt.begin(), Wt.end(), wt.begin() + ((size_t)t * 2 + 1) * tile);
        }
    };
    sample(0);
    for (int i = 0; i + 1 < in.T; i++) {
        sens_advance(in, Wt.data(), i);
        if (i >= 1) sens_advance(in, Wr.data(), i);
        sample(i + 1);
    }
}

// H[a][b] = sum_k (PSI[k][a] w_k) PSI[k][b] over ascending k, w_k = R_diag[k mod n_u] or 1 (R == nullptr); H is ld x ld, zero elsewhere.
// (A zero PSI[k][a] is skipped: its terms are zeros, which change no bit of a sum that starts at +0.)
inline void psi_gram(const BatchTableIn& in, const double* R, std::vector<double>& H) {
    const int Kw = in.Kw, ld = in.ld;
    H.assign((size_t)ld * ld, 0.0);
    for (int k = 0; k < in.rows(); k++) {
        const double* pr = in.psi + (size_t)k * Kw;
        for (int a = 0; a < Kw; a++) {
            if (pr[a] == 0.0) continue;
            const double pa = R ? pr[a] * R[k % in.n_u] : pr[a];
            for (int b = 0; b < Kw; b++) H[(size_t)a * ld + b] += pa * pr[b];
        }
    }
}

// Cholesky inverse of a symmetric positive matrix (row-major n x n); false if it is not positive
inline bool spd_inverse(std::vector<double>& A, int n) {
    std::vector<double> L((size_t)n * n, 0.0);
    for (int j = 0; j < n; j++) {
        double s = A[(size_t)j * n + j];
        for (int k = 0; k < j; k++) s -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(s > 0)) return false;
        const double ljj = std::sqrt(s);
        L[(size_t)j * n + j] = ljj;
        for (int i = j + 1; i < n; i++) {
            double t = A[(size_t)i * n + j];
            for (int k = 0; k < j; k++) t -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = t / ljj;
        }
    }
    std::vector<double> Li((size_t)n * n, 0.0);  // L^-1 (lower)
    for (int c = 0; c < n; c++) {
        Li[(size_t)c * n + c] = 1.0 / L[(size_t)c * n + c];
        for (int i = c + 1; i < n; i++) {
            double t = 0;
            for (int k = c; k < i; k++) t -= L[(size_t)i * n + k] * Li[(size_t)k * n + c];
            Li[(size_t)i * n + c] = t / L[(size_t)i * n + i];
        }
    }
    for (int i = 0; i < n; i++)  // A^-1 = L^-T L^-1
        for (int j = 0; j <= i; j++) {
            double t = 0;
            for (int k = i; k < n; k++) t += Li[(size_t)k * n + i] * Li[(size_t)k * n + j];
            A[(size_t)i * n + j] = A[(size_t)j * n + i] = t;
        }
    return true;
}

// out[i][:] += sum_q A[i][q] Z[q][:] over ascending q, zero A[i][q] skipped (A: rows x Kw, Z: Kw x m, out: rows x m)
inline void times_z(const double* A, size_t rows, int Kw, const std::vector<double>& Z, int m, std::vector<double>& out) {
    out.assign(rows * m, 0.0);
    const double* __restrict z = Z.data();  // (out and Z are different vectors: lets the compiler vectorise the row update)
    double* __restrict o = out.data();
    for (size_t i = 0; i < rows; i++)
        for (int q = 0; q < Kw; q++) {
            const double v = A[i * Kw + q];
            if (v == 0.0) continue;
            for (int j = 0; j < m; j++) o[i * m + j] += v * z[(size_t)q * m + j];
        }
}

// Narrow bases: PSI padded to ld columns, H0 and, where in.sens, the sensitivities and PSI'PSI.
struct NarrowTables {
    std::vector<double> psip, H0, wt, wr, pp;
};
inline void narrow_tables(const BatchTableIn& in, NarrowTables& t) {
    const int Kw = in.Kw, ld = in.ld;
    t.psip.assign((size_t)in.rows() * ld, 0.0);
    for (int k = 0; k < in.rows(); k++)
        for (int q = 0; q < Kw; q++) t.psip[(size_t)k * ld + q] = in.psi[(size_t)k * Kw + q];
    psi_gram(in, in.R_diag, t.H0);
    for (int q = Kw; q < ld; q++) t.H0[(size_t)q * ld + q] = 1.0;  // keeps H regular; the padded entries of dw come out 0
    if (!in.sens) { t.wt.clear(); t.wr.clear(); t.pp.clear(); return; }
    sens_tables(in, t.wt, t.wr);
    psi_gram(in, nullptr, t.pp);
}

// Wide bases (ld == Kw).  false: PSI'R PSI is not positive definite.
struct WideTables {
    std::vector<double> G, Et, PZ, ZPZ, h0inv;  // m x m, [n_kp][2][n_x] x m, (T-1) n_u x m, m x m, Kw x Kw (empty for the identity)
};
inline bool wide_tables(const BatchTableIn& in, WideTables& t) {
    const int Kw = in.Kw, m = in.n_kp * in.n_x, N = in.rows();
    std::vector<double> wt, V;
    sens_tables(in, wt, V);
    std::vector<double> Z((size_t)Kw * m, 0.0);  // H0^-1 V'
    t.h0inv.clear();
    if (!in.psi) {
        for (int q = 0; q < Kw; q++)
            for (int j = 0; j < m; j++) Z[(size_t)q * m + j] = V[(size_t)j * Kw + q] / in.R_diag[q % in.n_u];
    } else {
        psi_gram(in, in.R_diag, t.h0inv);
        if (!spd_inverse(t.h0inv, Kw)) return false;
        for (int q = 0; q < Kw; q++)
            for (int j = 0; j < m; j++) {
                double s = 0;
                for (int r = 0; r < Kw; r++) s += t.h0inv[(size_t)q * Kw + r] * V[(size_t)j * Kw + r];
                Z[(size_t)q * m + j] = s;
            }
    }
    times_z(V.data(), m, Kw, Z, m, t.G);
    for (int i = 0; i < m; i++)  // symmetric in exact arithmetic; the kernels rely on it
        for (int j = 0; j < i; j++) t.G[(size_t)i * m + j] = t.G[(size_t)j * m + i] = 0.5 * (t.G[(size_t)i * m + j] + t.G[(size_t)j * m + i]);
    times_z(wt.data(), (size_t)in.n_kp * 2 * in.n_x, Kw, Z, m, t.Et);
    if (!in.psi) t.PZ = Z;
    else times_z(in.psi, N, Kw, Z, m, t.PZ);
    t.ZPZ.assign((size_t)m * m, 0.0);
    const double* __restrict pz = t.PZ.data();
    double* __restrict zpz = t.ZPZ.data();
    for (int k = 0; k < N; k++)
        for (int i = 0; i < m; i++) {
            const double v = pz[(size_t)k * m + i];
            if (v == 0.0) continue;
            for (int j = 0; j < m; j++) zpz[(size_t)i * m + j] += v * pz[(size_t)k * m + j];
        }
    return true;
}

}  // namespace ilqr
