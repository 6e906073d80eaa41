// ilqr_multistart_kernels.hpp -- the kernels that join instances: definitions and launchers, included by ilqr_capi_kernels.cpp alone (inside no namespace).
// That file is compiled as HIP for the product library and as C++ for the host build of tests/tools/hostsim, so both get the kernels from one
// text and no list of files changes.  They are NOT in ilqr_kernels.hip: a kernel added there moves every kernel of that translation unit's code
// object, and the C3 bench line followed it -- 5.550 .. 5.575 ms per step against the parent's 5.529 .. 5.546 in one session, six runs each in
// rotating order, with these kernels at the end of that unit; 5.525 .. 5.554 with the unit left as it was (k_kp_derivs, which runs between the
// streaming kernels of every iteration and is bound by fetching its code, is the one kernel of that unit on the C3 path).  The C-ABI unit held
// no kernel before: nothing moves.  Plain C++; the lane moves of k_select_group are the helpers of ilqr_lanes.hpp and exist in the device build
// only (the host build runs its one-lane form).
//
//   k_adopt_rows       row gather [row][Bp_src] -> [row][Bp_dst] through an index; lanes run along the destination batch: every store of a wave
//                      is one whole 512-byte run, the loads are the gather
//   k_spread_controls  one lane per (instance, step): U0 += sigma_u z, z from ilqr_noise.hpp; sigma and the maps are kernel arguments (wave-uniform)
//   k_select_group     W lanes per group (1, 4, 16 or 64), the key (score, instance) reduced to its minimum
//   k_get_at           the gather of ilqr_problem_get_at into the natural layout, doubles and ints
// Offsets and flat thread indices are size_t throughout (B T n and G W may pass 2^31); an instance or group index is an int.
#pragma once
#ifndef ILQR_MULTISTART_KERNELS_TU
#error "ilqr_multistart_kernels.hpp holds definitions with external linkage: one translation unit (ilqr_capi_kernels.cpp) defines ILQR_MULTISTART_KERNELS_TU and includes it; every other one includes ilqr_multistart.hpp"
#endif
#include "ilqr_multistart.hpp"
#include "ilqr_noise.hpp"

#if defined(__HIPCC__)
#include "ilqr_lanes.hpp"
#endif

namespace ilqr {

__device__ __forceinline__ int ms_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// CUR: the source is a double-buffered array and cur[i] says which buffer holds instance i (the plan's controls); else s0 alone
template <bool CUR>
__global__ __launch_bounds__(256) void k_adopt_rows(const double* __restrict__ s0, const double* __restrict__ s1, const int* __restrict__ cur,
                                                    const int* __restrict__ index, double* __restrict__ dst, int B_dst, int Bp_dst, int B_src, int Bp_src) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;
    if (b >= B_dst) return;
    const int i = ms_clamp(index[b], B_src);
    const double* src = (CUR && cur[i]) ? s1 : s0;
    dst[(size_t)r * (size_t)Bp_dst + (size_t)b] = src[(size_t)r * (size_t)Bp_src + (size_t)i];
}

// Instance b = g S + s is member s of group g.  Pair j of counter (group_offset + g, member_offset + s, k, j) serves the user's control entries
// 2j and 2j + 1 (ilqr_noise.hpp: the stream of the closed-loop disturbances).  The product is rounded on its own, then one rounded add; an entry
// with sigma 0 is not touched and a pair with both sigmas 0 is not generated.  The global member 0 of a group keeps its controls.
// MAPPED: a chain of fewer than 7 joints, whose user entry i lives in device row u.dev[i]; else the identity
template <bool MAPPED>
__global__ __launch_bounds__(256) void k_spread_controls(double* __restrict__ U0, int B, int Bp, int S, ilqr_seeds sd, IndexMap u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int b = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (b >= B) return;
    const int g = b / S, s = b - g * S;
    const uint32_t member = sd.member_offset + (uint32_t)s;
    if (member == 0u) return;
    const int nuu = u.n_user, nud = u.n_dev;
    for (int j = 0; 2 * j < nuu; j++) {
        const int i0 = 2 * j, i1 = 2 * j + 1;
        const double s0 = sd.sigma_u[i0];
        const double s1 = i1 < nuu ? sd.sigma_u[i1] : 0.0;
        if (s0 == 0.0 && s1 == 0.0) continue;
        double z0, z1;
        noise_pair(sd.seed, sd.group_offset + (uint32_t)g, member, (uint32_t)k, (uint32_t)j, z0, z1);
        if (s0 != 0.0) {
            const double v = s0 * z0;
            double* e = U0 + ((size_t)k * (size_t)nud + (size_t)(MAPPED ? u.dev[i0] : i0)) * (size_t)Bp + (size_t)b;
            *e = *e + v;
        }
        if (s1 != 0.0) {
            const double v = s1 * z1;
            double* e = U0 + ((size_t)k * (size_t)nud + (size_t)(MAPPED ? u.dev[i1] : i1)) * (size_t)Bp + (size_t)b;
            *e = *e + v;
        }
    }
}

// The key of a candidate is (score, instance), ordered by the score as a double (-0 ties with +0) and then by the instance; an instance that is
// no candidate carries (+inf, INT_MAX), which every candidate precedes (a candidate's score is finite).  The order is total, so the minimum does
// not depend on the reduction tree: W lanes or one give the same winner.
struct MsKey { double score; int idx; };
__device__ __forceinline__ MsKey ms_min(const MsKey& a, const MsKey& b) {
    return (b.score < a.score || (b.score == a.score && b.idx < a.idx)) ? b : a;
}
constexpr int MS_NONE = 0x7fffffff;

#if defined(__HIPCC__)
template <int CTRL>
__device__ __forceinline__ void ms_step_dpp(MsKey& k, int& n) {
    MsKey o;
    o.score = dpp_f64<CTRL>(k.score);
    o.idx = __builtin_amdgcn_mov_dpp(k.idx, CTRL, 0xf, 0xf, false);
    n += __builtin_amdgcn_mov_dpp(n, CTRL, 0xf, 0xf, false);
    k = ms_min(k, o);
}
__device__ __forceinline__ void ms_step_rows(MsKey& k, int& n, int mask) {
    MsKey o;
    o.score = __shfl_xor(k.score, mask);
    o.idx = __shfl_xor(k.idx, mask);
    n += __shfl_xor(n, mask);
    k = ms_min(k, o);
}
#endif

// the minimum key and the candidate count over the W lanes of a group, in every one of them (the steps of quad_sum, oct_sum, row16_sum, wave_sum)
template <int W>
__device__ __forceinline__ void ms_reduce(MsKey& k, int& n) {
#if defined(__HIPCC__)
    if (W >= 4) { ms_step_dpp<0xB1>(k, n); ms_step_dpp<0x4E>(k, n); }     // quad_perm [1,0,3,2], [2,3,0,1]
    if (W >= 16) { ms_step_dpp<0x141>(k, n); ms_step_dpp<0x140>(k, n); }  // row_half_mirror, row_mirror
    if (W >= 64) { ms_step_rows(k, n, 16); ms_step_rows(k, n, 32); }
#else
    static_assert(W == 1, "the host build runs the one-lane form");
#endif
}

// W lanes per group, 256 / W groups per block; lane l of a group looks at members l, l + W, ...  Lanes of a group beyond G take part in the
// moves with no candidate and store nothing.
template <int W>
__global__ __launch_bounds__(256) void k_select_group(const double* __restrict__ score, const int* __restrict__ eligible, const int* __restrict__ status,
                                                      int G, int S, int* __restrict__ winner, double* __restrict__ best, int* __restrict__ n_candidates) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;   // G W may pass 2^31; t / W stays below G + 256 / W
    const int g = (int)(t / W), l = (int)(t % W);
    MsKey key{INFINITY, MS_NONE};
    int n = 0;
    if (g < G) {
        for (int s = l; s < S; s += W) {
            const int b = g * S + s;
            const double sc = score[b];
            const bool cand = (!eligible || eligible[b] != 0) && !(status[b] & (ILQR_STATUS_NONFINITE | ILQR_STATUS_SWEEP_IO)) && isfinite(sc);
            if (cand) { key = ms_min(key, MsKey{sc, b}); n++; }
        }
    }
    ms_reduce<W>(key, n);
    if (g < G && l == 0) {
        const bool none = key.idx == MS_NONE;
        if (winner) winner[g] = none ? g * S : key.idx;
        if (best) best[g] = none ? (double)NAN : key.score;
        if (n_candidates) n_candidates[g] = n;
    }
}

// V: double (X, U, cost) or int (iters, status); MAPPED: the rows are the user's and go through m to the device's (doubles only); cur may be null
template <class V, bool MAPPED>
__global__ __launch_bounds__(256) void k_get_at(const V* __restrict__ s0, const V* __restrict__ s1, const int* __restrict__ cur,
                                                const int* __restrict__ index, V* __restrict__ out, int n, int B_src, int Bp_src, IndexMap m) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;
    if (j >= n) return;
    int row = r;
    if (MAPPED) {
        const int o = r / m.n_user;
        row = o * m.n_dev + m.dev[r - o * m.n_user];
    }
    const int i = ms_clamp(index[j], B_src);
    const V* src = (cur && cur[i]) ? s1 : s0;
    out[(size_t)j * (size_t)gridDim.y + (size_t)r] = src[(size_t)row * (size_t)Bp_src + (size_t)i];
}

// ------------------------------------------------------------------------------------------------ launchers

void launch_adopt_rows(const double* s0, const double* s1, const int* cur, const int* index, double* dst, int rows, int B_dst, int Bp_dst, int B_src,
                       int Bp_src, hipStream_t st) {
    if (rows <= 0) return;
    const dim3 grid((B_dst + 255) / 256, rows), block(256);
    if (cur) hipLaunchKernelGGL((k_adopt_rows<true>), grid, block, 0, st, s0, s1, cur, index, dst, B_dst, Bp_dst, B_src, Bp_src);
    else hipLaunchKernelGGL((k_adopt_rows<false>), grid, block, 0, st, s0, s1, cur, index, dst, B_dst, Bp_dst, B_src, Bp_src);
}

void launch_spread_controls(double* U0, int B, int Bp, int T1, int group_size, const ilqr_seeds& seeds, const IndexMap& u, hipStream_t st) {
    const dim3 grid((B + 255) / 256, T1), block(256);
    if (u.n_user != u.n_dev) hipLaunchKernelGGL((k_spread_controls<true>), grid, block, 0, st, U0, B, Bp, group_size, seeds, u);
    else hipLaunchKernelGGL((k_spread_controls<false>), grid, block, 0, st, U0, B, Bp, group_size, seeds, u);
}

void launch_select_group(const double* score, const int* eligible, const int* status, int G, int group_size, int* winner, double* best,
                         int* n_candidates, hipStream_t st) {
    const int S = group_size;
#if defined(__HIPCC__)
    const int W = S <= 1 ? 1 : (S <= 4 ? 4 : (S <= 16 ? 16 : 64));
#else
    const int W = 1;
#endif
    const dim3 grid((unsigned)(((size_t)G * W + 255) / 256)), block(256);
    switch (W) {
#if defined(__HIPCC__)
        case 4: hipLaunchKernelGGL((k_select_group<4>), grid, block, 0, st, score, eligible, status, G, S, winner, best, n_candidates); break;
        case 16: hipLaunchKernelGGL((k_select_group<16>), grid, block, 0, st, score, eligible, status, G, S, winner, best, n_candidates); break;
        case 64: hipLaunchKernelGGL((k_select_group<64>), grid, block, 0, st, score, eligible, status, G, S, winner, best, n_candidates); break;
#endif
        default: hipLaunchKernelGGL((k_select_group<1>), grid, block, 0, st, score, eligible, status, G, S, winner, best, n_candidates); break;
    }
}

void launch_get_at(const double* s0, const double* s1, const int* cur, const int* index, double* out, int n, int B_src, int Bp_src, int rows,
                   const IndexMap* m, hipStream_t st) {
    if (rows <= 0) return;
    const dim3 grid((n + 255) / 256, rows), block(256);
    if (m) hipLaunchKernelGGL((k_get_at<double, true>), grid, block, 0, st, s0, s1, cur, index, out, n, B_src, Bp_src, *m);
    else hipLaunchKernelGGL((k_get_at<double, false>), grid, block, 0, st, s0, s1, cur, index, out, n, B_src, Bp_src, IndexMap{});
}

void launch_get_at_int(const int* src, const int* index, int* out, int n, int B_src, hipStream_t st) {
    hipLaunchKernelGGL((k_get_at<int, false>), dim3((n + 255) / 256, 1), dim3(256), 0, st, src, (const int*)nullptr, (const int*)nullptr, index, out, n, B_src, 0, IndexMap{});
}

}  // namespace ilqr
