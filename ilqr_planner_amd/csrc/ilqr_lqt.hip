// ilqr_lqt.hip -- batched linear-quadratic tracking (solver::LQT, reference src/solver/lqt.cpp) on the f64 units of gfx950
//
// LQT tracks targets mu_t, t = 0..N-1, with x' = A x + B u and the cost sum_t (x_t - mu_t)' Q_t (x_t - mu_t) + sum_t u_t' R u_t, R = r I.
// The dynamic-programming form (lqt.cpp:29-53), with P_{N-1} = Q_{N-1}, d_{N-1} = 0 and, for t = N-1 .. 1,
//     S_t = B' P_t B + R          L_t = S_t^-1 B' P_t        H_t = S_t^-1 B'        Acl_t = A - B L_t A
//     P_{t-1} = Q_{t-1} + Acl_t' P_t A                       (= Q - A'(P B S^-1 B' P - P) A)
//     d_{t-1} = Acl_t' (P_t (A mu_{t-1} - mu_t) + d_t)       (= (A' - A' P B S^-1 B')(P (A mu - mu') + d))
// The command of lqt.cpp:102-120 at tau = t + 1, u = K (mu_tau - x) + f with K = L_tau A and f = -L_tau (A mu_tau - mu_tau) - H_tau d_tau, is
//     u = L_tau (mu_tau - A x) - H_tau d_tau,
// which is also the optimal law for x_t (K (mu_t - x) - L (A mu_t - mu_tau) - H d reduces to the same expression): the reference's use of
// mu_tau in both places cancels.  So the command kernel and the rollout of solve_lin_al share one step.
//
// Kernels
//   k_lqt_chain    one wave per Riccati chain, the whole horizon in one launch.  n <= 16 is padded to one v_mfma_f64_16x16x4_f64 tile;
//                  every product of a step is a chain of 2 or 4 MFMAs on registers, S (m <= 8, padded with an identity tail to 8) goes through
//                  LDS once and is inverted in registers (quu_pivots, ilqr_pivots.hpp).  Writes P_t, L_t, H_t; for a shared chain also
//                  W_t = Acl_t' (the affine sweep's matrix); for per-instance precisions the d_t recursion rides along (fused).
//   k_lqt_affine   d_t of B instances from the shared chain: NP lanes per instance (lane i owns row i), P_t / W_t rows batch-uniform (cache
//                  resident), mu read once, d written once.
//   k_lqt_rollout  solve_lin_al's forward pass from x_0 = mu_0: U, X.
//   k_lqt_command  the command of B instances at one step.
// No kernel's choice depends on the batch size, and none has data-dependent addressing: a NaN in the inputs gives NaN outputs.
#include "ilqr_lqt.hpp"
#include "ilqr_pivots.hpp"

namespace ilqr {

// Every block is one wave: LDS accesses of a wave complete in issue order, so a compiler barrier orders them.  (__syncthreads would add a
// workgroup release fence -- s_waitcnt vmcnt(0) on the global stores of the step -- and put the HBM store latency on the chain twice a step.)
#define LQT_LDS_ORDER() asm volatile("" ::: "memory")

typedef double d4l_t __attribute__((ext_vector_type(4)));

// The f64 MFMA C/D layout: lane (h = l >> 4, c = l & 15) holds M[h + 4 r][c] in register r.  Given X and Y in that layout, feeding register r of
// X as the A operand and register r of Y as the B operand of k-step r computes X' Y -- no shuffles between the products of a step.
__device__ __forceinline__ d4l_t mmt4(const d4l_t& X, const d4l_t& Y, d4l_t acc) {
#pragma unroll
    for (int r = 0; r < 4; r++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X[r], Y[r], acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ d4l_t zero4() { return d4l_t{0.0, 0.0, 0.0, 0.0}; }
// Global loads and stores are branch-free: a lane off the matrix loads entry 0 and drops it, and stores to its slot of the dump row
// (LqtDev::dump).  Exec-mask branches around them would make the compiler's wait-count tracking give up at every join (s_waitcnt vmcnt(0):
// each step would wait for its own loads and for the stores of the step before; the rollout at n = 14, B = 4096 took 795 us that way, 410 us now).
__device__ __forceinline__ double ld_or0(const double* M, bool ok, size_t i) {
    const double v = M[ok ? i : 0];
    return ok ? v : 0.0;
}
__device__ __forceinline__ void st_or_dump(double* M, bool ok, size_t i, double* dump, double v) { *(ok ? M + i : dump + threadIdx.x) = v; }
// M[rows][cols] (leading dimension ld) into the C layout, zero-padded
__device__ __forceinline__ d4l_t load_c(const double* M, int rows, int cols, int ld, int h, int c) {
    d4l_t v;
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = ld_or0(M, h + 4 * r < rows && c < cols, (h + 4 * r) * ld + c);
    return v;
}
// M' into the C layout (M is cols x rows with leading dimension ld)
__device__ __forceinline__ d4l_t load_ct(const double* M, int rows, int cols, int ld, int h, int c) {
    d4l_t v;
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = ld_or0(M, h + 4 * r < rows && c < cols, c * ld + h + 4 * r);
    return v;
}
__device__ __forceinline__ void store_c(double* M, const d4l_t& v, int rows, int cols, int h, int c, double* dump) {
#pragma unroll
    for (int r = 0; r < 4; r++) st_or_dump(M, h + 4 * r < rows && c < cols, (h + 4 * r) * cols + c, dump, v[r]);
}
// a vector as column 0 of the C layout
__device__ __forceinline__ d4l_t load_col(const double* v, int n, int h, int c) {
    d4l_t o;
#pragma unroll
    for (int r = 0; r < 4; r++) o[r] = ld_or0(v, c == 0 && h + 4 * r < n, h + 4 * r);
    return o;
}
__device__ __forceinline__ void store_col(double* v, const d4l_t& o, int n, int h, int c, double* dump) {
#pragma unroll
    for (int r = 0; r < 4; r++) st_or_dump(v, c == 0 && h + 4 * r < n, h + 4 * r, dump, o[r]);
}

template <bool FUSED>
__global__ __launch_bounds__(64) void k_lqt_chain(LqtDev a) {
    __shared__ double sS[8][9];
    const int l = threadIdx.x, h = l >> 4, c = l & 15;
    const int ch = blockIdx.x;
    const int n = a.n, m = a.m, N = a.N;
    const size_t nn = (size_t)n * n, mn = (size_t)m * n;
    const double* Q = a.Q + ch * N * nn;
    double* P = a.P + ch * N * nn;
    double* L = a.L + ch * N * mn;
    double* H = a.H + ch * N * mn;
    const double* mu = a.mu + ch * N * (size_t)n;  // FUSED: chain ch is instance ch
    double* dd = a.d + ch * N * (size_t)n;

    const d4l_t Ac = load_c(a.A, n, n, n, h, c), ATc = load_ct(a.A, n, n, n, h, c);
    const d4l_t Bc = load_c(a.Bm, n, m, m, h, c), BTc = load_ct(a.Bm, m, n, m, h, c);
    double nm1[8];  // quu_pivots: -1 in the lanes whose row is pivot k's
#pragma unroll
    for (int k = 0; k < 8; k++) nm1[k] = ((c & 7) == k) ? -1.0 : 0.0;
    const double sdiag = (c < m) ? a.r : 1.0;  // S + R, and an identity tail from m to 8 (B's padded columns are 0)

    d4l_t Pc = load_c(Q + (N - 1) * nn, n, n, n, h, c);
    d4l_t Dv = zero4();
    if (FUSED) store_col(dd + (size_t)(N - 1) * n, Dv, n, h, c, a.dump);
    for (int t = N - 1; t >= 0; t--) {
        // loads of the next step first: waiting for them then waits only for stores of earlier steps (vmcnt counts both, in order)
        const int tp = t > 0 ? t - 1 : 0;
        const d4l_t Qn = load_c(Q + tp * nn, n, n, n, h, c);
        d4l_t Mp = zero4(), Mt = zero4();
        if (FUSED) {
            Mp = load_col(mu + (size_t)tp * n, n, h, c);
            Mt = load_col(mu + (size_t)t * n, n, h, c);
        }
        store_c(P + t * nn, Pc, n, n, h, c, a.dump);
        const d4l_t PB = mmt4(Pc, Bc, zero4()), PA = mmt4(Pc, Ac, zero4());  // P symmetric: P' B = P B
        const d4l_t S = mmt4(Bc, PB, zero4()), BtP = mmt4(Bc, Pc, zero4()), BtPA = mmt4(Bc, PA, zero4());
        if (c < 8) {
            sS[h][c] = S[0] + (h == c ? sdiag : 0.0);
            sS[h + 4][c] = S[1] + (h + 4 == c ? sdiag : 0.0);
        }
        LQT_LDS_ORDER();
        double srow[8];
#pragma unroll
        for (int k = 0; k < 8; k++) srow[k] = sS[c & 7][k];
        LQT_LDS_ORDER();
        double myrc = 0.0;
        quu_pivots<8>(srow, nm1, myrc);  // afterwards -myrc * srow = row (c & 7) of S^-1
        // A operand of k-step s: S^-1[c][4 s + h] (rows c < 8; the copies in lanes 8..15 feed zeros)
        const double msc = (c < 8) ? -myrc : 0.0;
        const double lo01 = (h & 1) ? srow[1] : srow[0], lo23 = (h & 1) ? srow[3] : srow[2], hi01 = (h & 1) ? srow[5] : srow[4],
                     hi23 = (h & 1) ? srow[7] : srow[6];
        const double sa0 = ((h & 2) ? lo23 : lo01) * msc, sa1 = ((h & 2) ? hi23 : hi01) * msc;
        d4l_t Lc = zero4(), Hc = zero4(), Kc = zero4();
        Lc = __builtin_amdgcn_mfma_f64_16x16x4f64(sa0, BtP[0], Lc, 0, 0, 0);
        Lc = __builtin_amdgcn_mfma_f64_16x16x4f64(sa1, BtP[1], Lc, 0, 0, 0);
        Kc = __builtin_amdgcn_mfma_f64_16x16x4f64(sa0, BtPA[0], Kc, 0, 0, 0);
        Kc = __builtin_amdgcn_mfma_f64_16x16x4f64(sa1, BtPA[1], Kc, 0, 0, 0);
        Hc = __builtin_amdgcn_mfma_f64_16x16x4f64(sa0, BTc[0], Hc, 0, 0, 0);
        Hc = __builtin_amdgcn_mfma_f64_16x16x4f64(sa1, BTc[1], Hc, 0, 0, 0);
        store_c(L + t * mn, Lc, m, n, h, c, a.dump);
        store_c(H + t * mn, Hc, m, n, h, c, a.dump);
        if (t == 0) break;
        // Acl = A - B K: (B')' K over the m <= 8 rows of K, two k-steps
        d4l_t Acl = Ac;
        Acl = __builtin_amdgcn_mfma_f64_16x16x4f64(-BTc[0], Kc[0], Acl, 0, 0, 0);
        Acl = __builtin_amdgcn_mfma_f64_16x16x4f64(-BTc[1], Kc[1], Acl, 0, 0, 0);
        if (!FUSED) {  // W_t = Acl' row-major: lane (h, c) owns Acl[h + 4 r][c] = W[c][h + 4 r]
#pragma unroll
            for (int r = 0; r < 4; r++)
                st_or_dump(a.W, h + 4 * r < n && c < n, t * nn + c * n + h + 4 * r, a.dump, Acl[r]);
        }
        if (FUSED) {
            const d4l_t E = mmt4(ATc, Mp, -Mt);  // A mu_{t-1} - mu_t
            const d4l_t Z = mmt4(Pc, E, Dv);                                                                                   // P_t e + d_t
            Dv = mmt4(Acl, Z, zero4());                                                                                        // d_{t-1}
            store_col(dd + (size_t)(t - 1) * n, Dv, n, h, c, a.dump);
        }
        Pc = mmt4(Acl, PA, Qn);  // P_{t-1} = Q_{t-1} + Acl' P_t A
    }
}

// ---- lane-group kernels: NP lanes per instance, lane i of a group owns state row i (i < n) and control row i (i < m).  Lanes of an instance
// trade vectors through LDS (one wave per block: the barriers only order the LDS accesses).  Instances past B run on a clamped index and store
// nothing, so every lane reaches every barrier.
struct Lane {
    int l, g0, i, b, bb;
    bool live;
};
template <int NP>
__device__ __forceinline__ Lane lane_of(int B) {
    Lane o;
    o.l = threadIdx.x;
    o.i = o.l % NP;
    o.g0 = o.l - o.i;
    o.b = blockIdx.x * (64 / NP) + o.l / NP;
    o.live = o.b < B;
    o.bb = o.live ? o.b : B - 1;
    return o;
}

template <int NP>
__global__ __launch_bounds__(64) void k_lqt_affine(LqtDev a) {
    __shared__ double sx[64];
    const int n = a.n, N = a.N;
    const Lane q = lane_of<NP>(a.B);
    const bool own = q.i < n;
    const int ii = own ? q.i : 0;
    double arow[NP];
#pragma unroll
    for (int j = 0; j < NP; j++) arow[j] = ld_or0(a.A, j < n, ii * n + j);
    const double* mu = a.mu + (size_t)q.bb * N * n;
    double* dd = a.d + (size_t)q.bb * N * n;
    double di = 0.0;
    st_or_dump(dd, q.live && own, (size_t)(N - 1) * n + q.i, a.dump, 0.0);
    for (int t = N - 2; t >= 0; t--) {
        const double* mt = mu + (size_t)t * n;
        const double* Pr = a.P + (size_t)(t + 1) * n * n + ii * n;
        const double* Wr = a.W + (size_t)(t + 1) * n * n + ii * n;
        double e = 0.0;
#pragma unroll
        for (int j = 0; j < NP; j++) e = fma(arow[j], ld_or0(mt, j < n, j), e);  // (arow[j] = 0 for j >= n)
        e = own ? e - mt[n + ii] : 0.0;  // (A mu_t - mu_{t+1})_i
        sx[q.l] = e;
        LQT_LDS_ORDER();
        double z = di;
#pragma unroll
        for (int j = 0; j < NP; j++) z = fma(ld_or0(Pr, j < n, j), sx[q.g0 + j], z);
        LQT_LDS_ORDER();
        sx[q.l] = z;
        LQT_LDS_ORDER();
        double nd = 0.0;
#pragma unroll
        for (int j = 0; j < NP; j++) nd = fma(ld_or0(Wr, j < n, j), sx[q.g0 + j], nd);
        LQT_LDS_ORDER();
        di = own ? nd : 0.0;
        st_or_dump(dd, q.live && own, (size_t)t * n + q.i, a.dump, di);
    }
}

// One step of the law u = L_tau (mu_tau - A x) - H_tau d_tau for the lane's instance; x is this lane's coordinate (0 beyond n).
// Returns u_i (0 for i >= m); ax receives (A x)_i.
template <int NP>
__device__ __forceinline__ double lqt_step(const LqtDev& a, const Lane& q, double* sx, const double (&arow)[NP], double x, int tau, double& ax) {
    const int n = a.n, m = a.m, N = a.N;
    const int ch = a.chains == 1 ? 0 : q.bb;
    const bool own = q.i < n, ctl = q.i < m;
    const int ii = own ? q.i : 0, k = ctl ? q.i : 0;
    const double* Lr = a.L + ((size_t)ch * N + tau) * m * n + k * n;
    const double* Hr = a.H + ((size_t)ch * N + tau) * m * n + k * n;
    const double* dt = a.d + ((size_t)q.bb * N + tau) * n;
    const double* mt = a.mu + ((size_t)q.bb * N + tau) * n;
    sx[q.l] = x;
    LQT_LDS_ORDER();
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NP; j++) s = fma(arow[j], sx[q.g0 + j], s);
    LQT_LDS_ORDER();
    ax = own ? s : 0.0;
    sx[q.l] = own ? mt[ii] - s : 0.0;  // y = mu_tau - A x (0 in lanes i >= n)
    LQT_LDS_ORDER();
    double u = 0.0;
#pragma unroll
    for (int j = 0; j < NP; j++) u = fma(ld_or0(Lr, j < n, j), sx[q.g0 + j], u);
#pragma unroll
    for (int j = 0; j < NP; j++) u = fma(-ld_or0(Hr, j < n, j), ld_or0(dt, j < n, j), u);
    LQT_LDS_ORDER();
    return ctl ? u : 0.0;
}

template <int NP>
__device__ __forceinline__ void lane_rows(const LqtDev& a, const Lane& q, double (&arow)[NP], double (&brow)[8]) {
    const int n = a.n, m = a.m;
    const int ii = q.i < n ? q.i : 0;
#pragma unroll
    for (int j = 0; j < NP; j++) arow[j] = ld_or0(a.A, j < n, ii * n + j);
#pragma unroll
    for (int k = 0; k < 8; k++) brow[k] = ld_or0(a.Bm, k < m, ii * m + k);
}

template <int NP>
__global__ __launch_bounds__(64) void k_lqt_rollout(LqtDev a) {
    __shared__ double sx[64];
    const int n = a.n, m = a.m, N = a.N;
    const Lane q = lane_of<NP>(a.B);
    const bool own = q.i < n;
    double arow[NP], brow[8];
    lane_rows<NP>(a, q, arow, brow);
    double* X = a.X + (size_t)q.bb * N * n;
    double* U = a.U + (size_t)q.bb * (N - 1) * m;
    double x = own ? a.mu[(size_t)q.bb * N * n + q.i] : 0.0;  // x_0 = mu_0
    if (q.live && own) X[q.i] = x;
    for (int t = 0; t + 1 < N; t++) {
        double ax;
        const double u = lqt_step<NP>(a, q, sx, arow, x, t + 1, ax);
        sx[q.l] = u;
        LQT_LDS_ORDER();
        double bu = 0.0;
#pragma unroll
        for (int k = 0; k < 8; k++) bu = fma(brow[k], sx[q.g0 + (k < NP ? k : 0)], bu);  // (brow[k] = 0 for k >= m)
        LQT_LDS_ORDER();
        x = own ? ax + bu : 0.0;
        st_or_dump(U, q.live && q.i < m, (size_t)t * m + q.i, a.dump, u);
        st_or_dump(X, q.live && own, (size_t)(t + 1) * n + q.i, a.dump, x);
    }
}

template <int NP>
__global__ __launch_bounds__(64) void k_lqt_command(LqtDev a, int tau, const double* __restrict__ xin, double* __restrict__ uout) {
    __shared__ double sx[64];
    const int n = a.n, m = a.m;
    const Lane q = lane_of<NP>(a.B);
    double arow[NP], brow[8];
    lane_rows<NP>(a, q, arow, brow);
    const double x = q.i < n ? xin[(size_t)q.bb * n + q.i] : 0.0;
    double ax;
    const double u = lqt_step<NP>(a, q, sx, arow, x, tau, ax);
    if (q.live && q.i < m) uout[(size_t)q.b * m + q.i] = u;
}

// ---- launchers
static unsigned groups_grid(int B, int np) { return (unsigned)((B + 64 / np - 1) / (64 / np)); }

void launch_lqt_chain(const LqtDev& a, hipStream_t s) {
    if (a.chains == 1) hipLaunchKernelGGL(k_lqt_chain<false>, dim3(1), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(k_lqt_chain<true>, dim3(a.chains), dim3(64), 0, s, a);
}
void launch_lqt_affine(const LqtDev& a, hipStream_t s) {
    const int np = lqt_group(a.n, a.m);
    const dim3 g(groups_grid(a.B, np)), b(64);
    if (np == 4) hipLaunchKernelGGL(k_lqt_affine<4>, g, b, 0, s, a);
    else if (np == 8) hipLaunchKernelGGL(k_lqt_affine<8>, g, b, 0, s, a);
    else hipLaunchKernelGGL(k_lqt_affine<16>, g, b, 0, s, a);
}
void launch_lqt_rollout(const LqtDev& a, hipStream_t s) {
    const int np = lqt_group(a.n, a.m);
    const dim3 g(groups_grid(a.B, np)), b(64);
    if (np == 4) hipLaunchKernelGGL(k_lqt_rollout<4>, g, b, 0, s, a);
    else if (np == 8) hipLaunchKernelGGL(k_lqt_rollout<8>, g, b, 0, s, a);
    else hipLaunchKernelGGL(k_lqt_rollout<16>, g, b, 0, s, a);
}
void launch_lqt_command(const LqtDev& a, int tau, const double* x, double* u, hipStream_t s) {
    const int np = lqt_group(a.n, a.m);
    const dim3 g(groups_grid(a.B, np)), b(64);
    if (np == 4) hipLaunchKernelGGL(k_lqt_command<4>, g, b, 0, s, a, tau, x, u);
    else if (np == 8) hipLaunchKernelGGL(k_lqt_command<8>, g, b, 0, s, a, tau, x, u);
    else hipLaunchKernelGGL(k_lqt_command<16>, g, b, 0, s, a, tau, x, u);
}

}  // namespace ilqr
