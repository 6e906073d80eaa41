// ilqr_clearance_kernels.hpp -- the clearance kernels: definitions and launchers, included by ilqr_capi_kernels.cpp alone (inside no namespace), for the
// reasons at the top of ilqr_multistart_kernels.hpp: that file is compiled as HIP for the product library and as C++ for the host build of
// tests/tools/hostsim, so both get the kernels from one text and no list of files changes, and no kernel of the .hip units moves.  Plain C++ without
// lane communication: the host build runs the very same code.
//
//   clr_state    THE per-state function, shared by both entry points: the walk over the descriptor's segments (one rolled copy of the joint step,
//                pose only, as the rolled form of fk<false>), the spheres by a cursor along the chain, the obstacle and plane loops and the key
//                update; the self pairs of a sphere behind its planes, against the anchors' centres kept in registers.  Contraction is off, so the two callers -- which differ only in how a joint position is loaded -- return the same bytes
//                for the same states.  A joint position is loaded when the walk reaches its joint: no register array, nothing indexed.
//   (k_clr_plan_self, k_clr_traj_self: the same two with clr_state<true>, launched for a geometry with self pairs)
//   k_clr_plan   the plan where it lies: lanes along the batch (every load of a wave is one whole 512-byte run of a [row][Bp] row), steps on blockIdx.y
//   k_clr_traj   natural layout: lanes along the flat (trajectory, step) index
//   k_clr_fold   one lane per trajectory: its keys in ascending step order under the total order of include/ilqr_hip.h
//   k_clr_stats  one lane per group: clr_min of its trajectories in index order
// The workspace holds 12 bytes per (trajectory, step): the clearance and sphere | obstacle << 5.
#pragma once
#ifndef ILQR_CLEARANCE_KERNELS_TU
#error "ilqr_clearance_kernels.hpp holds definitions with external linkage: one translation unit (ilqr_capi_kernels.cpp) defines ILQR_CLEARANCE_KERNELS_TU and includes it; every other one includes ilqr_clearance.hpp"
#endif
#include "ilqr_clearance.hpp"

namespace ilqr {

struct ClrKey { double clr; int code; };   // a bad step: (NaN, -1); a step without an active obstacle or plane: (+inf, -1)

// q(j): the position of joint j of this lane's state.  obs: this trajectory's set, [n_obs][4].
// SELF: the form with the self-pair block; the launchers take it only for a geometry that has pairs (ClrArgs::n_anchor), so a geometry without
// them runs the code it ran before there were any.
template <bool SELF, class Q>
__device__ __forceinline__ ClrKey clr_state(const ClrGeom& g, const double* __restrict__ obs, int n_obs, Q q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
    double W[SELF ? ILQR_CLR_MAX_ANCHOR : 1][3];   // the anchors' centres (self pairs); a slot is written before any pair reads it
    if (SELF) {
#pragma unroll
        for (int t = 0; t < ILQR_CLR_MAX_ANCHOR; t++) W[t][0] = W[t][1] = W[t][2] = 0;
    }
    const int n_anchor = SELF ? g.n_anchor : 0, self_base = n_obs + g.n_planes;
    ClrKey key{INFINITY, -1};
    bool bad = false;
    int cur = 0;
    const int n_sph = g.n_sph, n_planes = g.n_planes;
#pragma unroll 1
    for (int s = -1; s < g.n_walk; s++) {   // link -1 is the base: its spheres come before the first segment
        if (s >= 0) {
            const double x = g.seg_xyz[s][0], y = g.seg_xyz[s][1], z = g.seg_xyz[s][2];
#pragma unroll
            for (int i = 0; i < 3; i++) p[i] = p[i] + ((R[3 * i] * x + R[3 * i + 1] * y) + R[3 * i + 2] * z);
            double Rn[9];
            clr_mul(R, g.seg_R[s], Rn);
            const int jn = g.seg_joint[s];   // wave-uniform
            if (jn >= 0) {
                const double qj = q(jn);
                bad = bad || !isfinite(qj);
                const double ax = g.seg_axis[s][0], ay = g.seg_axis[s][1], az = g.seg_axis[s][2];
                double st, ct;
                sincos(qj, &st, &ct);
                const double vt = 1 - ct;
                const double Rq[9] = {ct + vt * ax * ax,      -az * st + vt * ax * ay, ay * st + vt * ax * az,
                                      az * st + vt * ax * ay, ct + vt * ay * ay,       -ax * st + vt * ay * az,
                                      -ay * st + vt * ax * az, ax * st + vt * ay * az, ct + vt * az * az};
                clr_mul(Rn, Rq, R);
            } else {
#pragma unroll
                for (int i = 0; i < 9; i++) R[i] = Rn[i];
            }
        }
#pragma unroll 1
        for (; cur < n_sph && g.sph_link[cur] == s; cur++) {
            const double cx = g.sph_c[cur][0], cy = g.sph_c[cur][1], cz = g.sph_c[cur][2], r = g.sph_r[cur];
            const double wx = p[0] + ((R[0] * cx + R[1] * cy) + R[2] * cz);
            const double wy = p[1] + ((R[3] * cx + R[4] * cy) + R[5] * cz);
            const double wz = p[2] + ((R[6] * cx + R[7] * cy) + R[8] * cz);
#pragma unroll 1
            for (int j = 0; j < n_obs; j++) {
                const double oR = obs[4 * (size_t)j + 3];
                if (oR < 0) continue;   // an unused slot
                const double dx = wx - obs[4 * (size_t)j], dy = wy - obs[4 * (size_t)j + 1], dz = wz - obs[4 * (size_t)j + 2];
                const double d = (sqrt((dx * dx + dy * dy) + dz * dz) - r) - oR;
                if (d < key.clr) { key.clr = d; key.code = cur | (j << 5); }
            }
#pragma unroll 1
            for (int l = 0; l < n_planes; l++) {
                const double d = ((((g.plane_n[l][0] * wx + g.plane_n[l][1] * wy) + g.plane_n[l][2] * wz)) - g.plane_d[l]) - r;
                if (d < key.clr) { key.clr = d; key.code = cur | ((n_obs + l) << 5); }
            }
            if constexpr (SELF) if (n_anchor) {   // wave-uniform, as mask and slot are
                const int mask = g.self_mask[cur];
#pragma unroll 1
                for (int t = 0; t < n_anchor; t++) {   // the anchors ascending
                    if (!(mask >> t & 1)) continue;
                    double c[3];
                    clr_anchor_get(W, t, c);
                    const double dx = wx - c[0], dy = wy - c[1], dz = wz - c[2];
                    const double d = (sqrt((dx * dx + dy * dy) + dz * dz) - r) - g.anc_r[t];
                    if (d < key.clr) { key.clr = d; key.code = cur | ((self_base + g.anc_sph[t]) << 5); }
                }
                clr_anchor_put(W, g.self_slot[cur], wx, wy, wz);
            }
        }
    }
    if (bad) { key.clr = (double)NAN; key.code = -1; }
    return key;
}

template <bool SELF>
__device__ __forceinline__ void clr_plan_body(const double* __restrict__ X0, const double* __restrict__ X1, const int* __restrict__ cur, int NX, int Bp, int k0,
                                              const ClrArgs& a) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int k = k0 + (int)blockIdx.y;
    if (b >= a.n) return;
    const double* x = (cur[b] ? X1 : X0) + (size_t)k * (size_t)NX * (size_t)Bp + (size_t)b;
    const size_t Bps = (size_t)Bp;
    const ClrKey key = clr_state<SELF>(*a.geom, a.obs + (size_t)(b / a.traj_per_set) * (size_t)a.n_obs * 4, a.n_obs,
                                       [&](int j) { return x[(size_t)a.qrow[j] * Bps]; });
    const size_t w = (size_t)k * (size_t)a.n + (size_t)b;
    a.ws_clr[w] = key.clr;
    a.ws_code[w] = key.code;
}
__global__ __launch_bounds__(256) void k_clr_plan(const double* __restrict__ X0, const double* __restrict__ X1, const int* __restrict__ cur, int NX, int Bp,
                                                  int k0, ClrArgs a) {
    clr_plan_body<false>(X0, X1, cur, NX, Bp, k0, a);
}
__global__ __launch_bounds__(256) void k_clr_plan_self(const double* __restrict__ X0, const double* __restrict__ X1, const int* __restrict__ cur, int NX,
                                                       int Bp, int k0, ClrArgs a) {
    clr_plan_body<true>(X0, X1, cur, NX, Bp, k0, a);
}

template <bool SELF>
__device__ __forceinline__ void clr_traj_body(const double* __restrict__ X, int n_x, const ClrArgs& a) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;   // n T may pass 2^31
    if (t >= (size_t)a.n * (size_t)a.T) return;
    const int i = (int)(t / (size_t)a.T);
    const double* x = X + t * (size_t)n_x;
    const ClrKey key = clr_state<SELF>(*a.geom, a.obs + (size_t)(i / a.traj_per_set) * (size_t)a.n_obs * 4, a.n_obs, [&](int j) { return x[a.qrow[j]]; });
    a.ws_clr[t] = key.clr;
    a.ws_code[t] = key.code;
}
__global__ __launch_bounds__(256) void k_clr_traj(const double* __restrict__ X, int n_x, ClrArgs a) { clr_traj_body<false>(X, n_x, a); }
__global__ __launch_bounds__(256) void k_clr_traj_self(const double* __restrict__ X, int n_x, ClrArgs a) { clr_traj_body<true>(X, n_x, a); }

// Steps ascend, so a strict `<` keeps the lowest step of equal clearances; sphere and obstacle were settled within the step.
__global__ __launch_bounds__(256) void k_clr_fold(double* __restrict__ ws_clr, const int* __restrict__ ws_code, int n, int T, size_t stride_i, size_t stride_k,
                                                  double margin, ilqr_clr_out out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double best = INFINITY;
    int bk = 0, bcode = -1, badk = -1, below = 0;
    for (int k = 0; k < T; k++) {
        const size_t w = (size_t)i * stride_i + (size_t)k * stride_k;
        const double c = ws_clr[w];
        if (out.clr) out.clr[(size_t)i * (size_t)T + (size_t)k] = c;
        if (c != c) {
            if (badk < 0) badk = k;
        } else {
            if (c < margin) below++;
            if (c < best) { best = c; bk = k; bcode = ws_code[w]; }
        }
    }
    const bool bad = badk >= 0;
    const double cmin = bad ? (double)NAN : best;
    if (out.clr_min) out.clr_min[i] = cmin;
    if (out.clr_at) {
        int* at = out.clr_at + (size_t)i * 3;
        at[0] = bad ? badk : bk;
        at[1] = (bad || bcode < 0) ? -1 : (bcode & 31);
        at[2] = (bad || bcode < 0) ? -1 : (bcode >> 5);
    }
    if (out.n_below) out.n_below[i] = below;
    if (out.eligible) out.eligible[i] = (!bad && best >= margin) ? 1 : 0;
    ws_clr[(size_t)i * stride_i] = cmin;   // the slot of step 0 of this trajectory, which no other lane reads: what k_clr_stats takes
}

__global__ __launch_bounds__(256) void k_clr_stats(const double* __restrict__ src, size_t stride, int n_groups, int group, double margin, double* __restrict__ stats) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    double sum = 0.0, mn = INFINITY;
    int cnt = 0, hit = 0, bad = 0;
    for (int s = 0; s < group; s++) {
        const double v = src[((size_t)g * (size_t)group + (size_t)s) * stride];
        if (v != v) { bad++; continue; }
        sum = sum + v;
        cnt++;
        if (v < mn) mn = v;
        if (v < margin) hit++;
    }
    double* o = stats + (size_t)g * ILQR_CLR_STATS;
    o[0] = cnt ? sum / (double)cnt : (double)NAN;
    o[1] = cnt ? mn : (double)NAN;
    o[2] = (double)hit;
    o[3] = (double)bad;
}

// ------------------------------------------------------------------------------------------------ launchers

void launch_clr_plan(const double* X0, const double* X1, const int* cur, int NX, int Bp, const ClrArgs& a, hipStream_t st) {
    for (int k0 = 0; k0 < a.T; k0 += 65535) {   // the y extent of a grid
        const int rows = a.T - k0 < 65535 ? a.T - k0 : 65535;
        if (a.n_anchor) hipLaunchKernelGGL(k_clr_plan_self, dim3((a.n + 255) / 256, rows), dim3(256), 0, st, X0, X1, cur, NX, Bp, k0, a);
        else hipLaunchKernelGGL(k_clr_plan, dim3((a.n + 255) / 256, rows), dim3(256), 0, st, X0, X1, cur, NX, Bp, k0, a);
    }
}

void launch_clr_traj(const double* X, int n_x, const ClrArgs& a, hipStream_t st) {
    const size_t total = (size_t)a.n * (size_t)a.T;
    if (a.n_anchor) hipLaunchKernelGGL(k_clr_traj_self, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, X, n_x, a);
    else hipLaunchKernelGGL(k_clr_traj, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, X, n_x, a);
}

void launch_clr_fold(const ClrArgs& a, size_t stride_i, size_t stride_k, double margin, const ilqr_clr_out& out, hipStream_t st) {
    hipLaunchKernelGGL(k_clr_fold, dim3((a.n + 255) / 256), dim3(256), 0, st, a.ws_clr, (const int*)a.ws_code, a.n, a.T, stride_i, stride_k, margin, out);
}

void launch_clr_stats(const double* src, size_t stride, int n_groups, int group, double margin, double* stats, hipStream_t st) {
    hipLaunchKernelGGL(k_clr_stats, dim3((n_groups + 255) / 256), dim3(256), 0, st, src, stride, n_groups, group, margin, stats);
}

}  // namespace ilqr
