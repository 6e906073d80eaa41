// ilqr_closed_loop.hip -- cooperative kernels of the batched closed-loop rollout (ilqr_problem_closed_loop) for gfx950 (MI355X), fp64.
//
// Why the generic kernel (k_closed_loop, ilqr_kernels.hip: one lane per (instance, sample), everything from global memory) cannot be the hot
// path: a lane-step reads its instance's gain record, 56 (n_x = n_u = 7) to 128 (n_x = 15, n_u = 8) load instructions, and the chain of steps
// is bound by memory instructions per step x latency / 64 in flight (the note at k_forward_wg, ilqr_kernels_wave.hip).  All samples of an
// instance ask for the same bytes.
//
// k_closed_loop_coop: a wave (= a workgroup) owns 64 / NS instances x NS samples.  Its 64 lanes together copy the records of `depth` steps of
// those instances -- K_k | d_k as one contiguous run per step, xbar_k and ubar_k of each instance's current buffer -- into LDS, one block of
// steps at a time; then every lane walks the block with its sample's state in registers and reads its instance's record back by same-address
// LDS reads (broadcasts; the record stride is odd, so different instances sit in different banks).  The plan is read from memory once per
// (instance, step, wave), not once per sample.  The block is loaded and then used: the loads of the next block do not yet overlap the steps
// of this one (the waves of a SIMD overlap each other's).
// FK stays out of the chain: the rollout sums the limit terms and stores state | control of every step-table entry, and k_closed_loop_kp, one
// lane per (instance, sample), adds the keypoint terms in step-table order -- the order the generic kernel adds them in, so the two agree bit
// for bit (a lane per entry would need a second pass for the ordered sum).
// Both kernels take every case of the descriptor (second limit set, shared steps, dead zones, object frames, joint keypoints): they call the
// functions of ilqr_closed_loop.hpp.  Layouts of 7-joint problems only; narrower chains take the generic kernel's mapped variant.
#include <type_traits>

#include "ilqr_closed_loop.hpp"

namespace ilqr {

#define NOUNR _Pragma("unroll 1")

// CON: judge the constraint rows (ilqr_problem_closed_loop_report_con; c.con_max is given).  A template argument like FF: as a run-time branch
// on c.con_max it cost the calls that do not ask 0.4 to 2.8 %.
template <class S, bool SYM, int NS, bool FF, bool CON>
__global__ __launch_bounds__(64) void k_closed_loop_coop(Bufs a, ClArgs c, int depth, double* __restrict__ kpx) {
    constexpr int NX = S::NX, NU = S::NU, NI = 64 / NS;
    constexpr int RS = SYM ? KD_SYM_RS : NU * kd_rowp(NX);   // doubles of a gain record in memory
    constexpr int STRIDE = cl_stride(S::KIND, S::ND);        // doubles between the staged records of two instances
    static_assert(RS + NX + NU <= STRIDE, "staged record");
    extern __shared__ double lds[];                          // [depth][NI][STRIDE]: record | xbar | ubar
    const DevDesc& d = *a.desc;
    const int lane = threadIdx.x, li = lane / NS;
    const int b0 = blockIdx.x * NI, b = b0 + li, s = blockIdx.y * NS + lane % NS;
    const bool valid = b < d.B && s < c.S;
    // lanes of the padding run along on pair 0 and on the last instance's plan and store nothing (the gain records of b0 .. b0 + NI - 1 < Bp exist)
    const int g = valid ? b * c.S + s : 0;
    const int bq = b < d.B ? b : d.B - 1;
    const int Bp = d.Bp, T = d.T, BS = d.B * c.S;
    const double sc = (a.iters[bq] > 0) ? a.alpha[bq] : 1.0;
    // this lane's part of the staging: entry lane / NI (+ 64 / NI per round) of xbar | ubar of instance b0 + lane % NI
    const int sinst = lane % NI, sb = b0 + sinst < d.B ? b0 + sinst : d.B - 1, scur = a.cur[sb];
    const double* sX = a.X[scur] + sb;
    const double* sU = a.U[scur] + sb;

    double x[NX], u[NU], xn[NX];
    {
        const double* X0 = a.X[a.cur[bq]] + bq;
        UNR for (int i = 0; i < NX; i++) x[i] = c.x0 ? c.x0[g * NX + i] : X0[(size_t)i * Bp];
    }
    const unsigned gb = c.b_off + (unsigned)b, gs = c.s_off + (unsigned)s;   // the counter of this lane's draws (padding lanes: any)
    if (c.noise) {
        double nz[NX];
        const unsigned on = noise_draw<NX, false, false>(c.seed, gb, gs, NOISE_STEP_START, c.sigma_x0, NX, nullptr, nz);
        UNR for (int i = 0; i < NX; i++) if ((on >> i) & 1u) x[i] += nz[i];
    }
    double lim = 0;
    ClCon con;
    int st = 0;
    NOUNR for (int k0 = 0; k0 < T - 1; k0 += depth) {
        const int nk = (T - 1 - k0 < depth) ? T - 1 - k0 : depth;
        __syncthreads();  // the previous block has been read
        NOUNR for (int j = 0; j < nk; j++) {
            const int k = k0 + j;
            double* slot = lds + (size_t)j * NI * STRIDE;
            const double* src = a.KD + ((size_t)k * Bp + b0) * RS;  // NI records, contiguous
            UNR for (int r = 0; r < (NI * RS + 63) / 64; r++) {
                const int idx = r * 64 + lane, in = idx / RS;
                if (idx < NI * RS) slot[in * STRIDE + (idx - in * RS)] = src[idx];
            }
            UNR for (int r = 0; r < (NX + NU + NS - 1) / NS; r++) {
                const int i = r * NS + lane / NI;
                if (i < NX + NU) slot[sinst * STRIDE + RS + i] = i < NX ? sX[((size_t)k * NX + i) * Bp] : sU[((size_t)k * NU + (i - NX)) * Bp];
            }
        }
        __syncthreads();
        NOUNR for (int j = 0; j < nk; j++) {
            const int k = k0 + j;
            const double* r = lds + ((size_t)j * NI + li) * STRIDE;
            // the draw of this step depends on no state: issued first, it fills the latency of the control / dynamics chain below
            double nz[NX];
            unsigned on = 0;
            if (c.noise) on = noise_draw<NX, false, false>(c.seed, gb, gs, (unsigned)k, c.sigma_w, NX, nullptr, nz);
            if (c.X && valid) { UNR for (int i = 0; i < NX; i++) c.X[(g * T + k) * NX + i] = x[i]; }
            cl_control<S>(r, SYM, FF, r + RS, r + RS + NX, 1, sc, x, u);
            if (c.U && valid) { UNR for (int i = 0; i < NU; i++) c.U[(g * (T - 1) + k) * NU + i] = u[i]; }
            if constexpr (CON) cl_con<S>(a, c.con_tol, k, x, u, con);
            lim += cl_limits<S>(d, x);
            if (st < d.steps.n && d.steps.t[st] == k) {  // uniform: state | control of the step-table entry for k_closed_loop_kp
                if (valid) {
                    double* o = kpx + (size_t)st * (NX + NU) * BS + g;
                    UNR for (int i = 0; i < NX; i++) o[(size_t)i * BS] = x[i];
                    UNR for (int i = 0; i < NU; i++) o[(size_t)(NX + i) * BS] = u[i];
                }
                st++;
            }
            dyn_step<S>(d, x, u, xn);
            if (c.noise) cl_disturb<NX, false>(c, g, k, T, NX, nullptr, on, nz, valid, xn);
            else if (c.w) { UNR for (int i = 0; i < NX; i++) xn[i] += c.w[(g * (T - 1) + k) * NX + i]; }
            UNR for (int i = 0; i < NX; i++) x[i] = xn[i];
        }
    }
    if (!valid) return;
    if (c.X) { UNR for (int i = 0; i < NX; i++) c.X[(g * T + T - 1) * NX + i] = x[i]; }
    lim += cl_limits<S>(d, x);
    if (st < d.steps.n && d.steps.t[st] == T - 1) {
        double* o = kpx + (size_t)st * (NX + NU) * BS + g;
        UNR for (int i = 0; i < NX; i++) o[(size_t)i * BS] = x[i];
        UNR for (int i = 0; i < NU; i++) o[(size_t)(NX + i) * BS] = 0.0;
    }
    if (c.lim_cost) c.lim_cost[g] = lim;  // uniform: only the report asks
    if constexpr (CON) cl_con_store(c, g, con);
    c.cost[g] = lim;
}

// J = limit terms + keypoint terms of the stored step-table entries, in table order: one lane per (instance, sample)
template <class S>
__global__ __launch_bounds__(64) void k_closed_loop_kp(Bufs a, int n_samples, const double* __restrict__ kpx, double* __restrict__ cost) {
    constexpr int NX = S::NX, NU = S::NU;
    const DevDesc& d = *a.desc;
    const int BS = d.B * n_samples;
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= BS) return;
    const int b = g / n_samples;
    double kpc = 0;
    NOUNR for (int st = 0; st < d.steps.n; st++) {
        const double* o = kpx + (size_t)st * (NX + NU) * BS + g;
        double x[NX], u[NU];
        UNR for (int i = 0; i < NX; i++) x[i] = o[(size_t)i * BS];
        UNR for (int i = 0; i < NU; i++) u[i] = o[(size_t)(NX + i) * BS];
        kpc = cl_kp_terms<S>(d, a, b, st, x, u, kpc);
    }
    cost[g] = cost[g] + kpc;
}

template <class S, bool SYM, int NS>
static void launch_ns(const Bufs& a, const ClArgs& c, int B, const ClosedLoopPlan& pl, double* kpx, hipStream_t st) {
    const dim3 grid((B + 64 / NS - 1) / (64 / NS), (c.S + NS - 1) / NS), block(64);
    auto go = [&](auto ff, auto con) {
        hipLaunchKernelGGL((k_closed_loop_coop<S, SYM, NS, decltype(ff)::value, decltype(con)::value>), grid, block, pl.lds_bytes, st, a, c, pl.depth, kpx);
    };
    if (c.with_ff) c.con_max ? go(std::true_type{}, std::true_type{}) : go(std::true_type{}, std::false_type{});
    else c.con_max ? go(std::false_type{}, std::true_type{}) : go(std::false_type{}, std::false_type{});
}
template <class S, bool SYM>
static void launch_sys(const Bufs& a, const ClArgs& c, int B, const ClosedLoopPlan& pl, double* kpx, hipStream_t st) {
    switch (pl.ns) {
        case 4: launch_ns<S, SYM, 4>(a, c, B, pl, kpx, st); break;
        case 8: launch_ns<S, SYM, 8>(a, c, B, pl, kpx, st); break;
        case 16: launch_ns<S, SYM, 16>(a, c, B, pl, kpx, st); break;
        case 32: launch_ns<S, SYM, 32>(a, c, B, pl, kpx, st); break;
        default: launch_ns<S, SYM, 64>(a, c, B, pl, kpx, st); break;
    }
    hipLaunchKernelGGL((k_closed_loop_kp<S>), dim3(((unsigned)B * c.S + 63) / 64), dim3(64), 0, st, a, c.S, kpx, c.cost);
}

void launch_closed_loop_coop(int kind, int nd, const Bufs& a, const ClArgs& c, int B, const ClosedLoopPlan& pl, double* kpx, hipStream_t st) {
    SysAll::dispatch(kind, nd, [&](auto s) {
        using S = decltype(s);
        if constexpr (S::NX == DOF) {  // the packed symmetric gain record exists for the single-integrator systems only
            if (a.kd_sym) return launch_sys<S, true>(a, c, B, pl, kpx, st);
        }
        launch_sys<S, false>(a, c, B, pl, kpx, st);
    });
}

}  // namespace ilqr
