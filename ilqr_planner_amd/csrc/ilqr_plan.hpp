// ilqr_plan.hpp -- which kernels run a Riccati solve (ILQRRecursive / AL_ILQR): one pure decision from the problem's shape, the batch size and
// the context's pins, consumed by solve_riccati (ilqr_capi_solve.cpp).  No HIP here: tests/cpp/plan_table_main.cpp checks the table on the host.
#pragma once

namespace ilqr {

// Batches of at least this many instances may be solved as two halves on two streams (solve_riccati): every kernel of an iteration is a
// chain of T dependent steps that leaves much of the machine idle at these batch sizes, so one half's sweep can run under the other
// half's forward pass and decision.  The first half is cut at a multiple of 64 instances (whole waves, whole 128-byte lines).
constexpr int SPLIT_MIN_BATCH = 2048;
constexpr int split_first_half(int B) { return (B / 2 + 63) / 64 * 64; }

// ---- what each cooperative kernel supports (system kind: 0 PosOrn, 1 PosOrnTime, 2 JointSpace, 3 JointSpaceTime; nd = nb_deriv)

// k_backward_si_dpp: single-integrator dynamics; the constraint rows are shared over k, touch no control and live in registers (at most 4)
constexpr bool backward_si_supported(int kind, int nd, bool al, int m, int per_step, bool con_state_only) {
    return (kind == 0 || kind == 2) && nd == 1 && (!al || (con_state_only && per_step == 0 && m <= 4));
}
// k_backward_mfma: every system but JointSpace-1 (which always has the closed form), at most 16 AL rows in LDS
constexpr bool backward_mfma_supported(int kind, int /*nd*/, bool al, int m) { return kind != 2 && (!al || m <= 16); }
// k_backward_rows: one lane per row of [P|p] needs n_x >= 8 (not PosOrn-1) and at most 16 AL rows; JointSpace-1 has the closed form
constexpr bool backward_rows_supported(int kind, int nd, bool al, int m) {
    return kind != 2 && !(kind == 0 && nd == 1) && (!al || m <= 16);
}
// k_forward_reg / k_forward_wg / k_forward_dpp: the linear line search of the single-integrator systems, one lane row per step size (at most 16)
constexpr bool forward_wave_supported(int kind, int nd, int n_alpha) { return (kind == 0 || kind == 2) && nd == 1 && n_alpha <= 16; }
// k_forward_lin: the linear line search of PosOrn-2, at most 16 step sizes
constexpr bool forward_lin_supported(int kind, int nd, int n_alpha) { return kind == 0 && nd == 2 && n_alpha <= 16; }
// k_init_roll_lti: every system -- the coordinates integrate independently given the step's dt
constexpr bool init_lti_supported(int kind, int nd) {
    return ((kind == 0 || kind == 1) && (nd == 1 || nd == 2)) || ((kind == 2 || kind == 3) && nd == 1);
}

// The dense cooperative path of a problem with obstacle terms (RiccatiPlan::obs_dense): the single-integrator systems, every stage's l_x, l_xx
// precomputed (k_stage_dense), k_backward_si_dpp<.., SW_DENSE> on lone waves, the wave rollouts with the per-step-size obstacle cost (k_obs_ls).
constexpr bool obs_coop_supported(int kind, int nd, bool al, int m, int per_step, bool con_state_only, int n_alpha) {
    return backward_si_supported(kind, nd, al, m, per_step, con_state_only) && forward_wave_supported(kind, nd, n_alpha);
}

// number of step sizes the do/while of ILQRRecursive.cpp:101-155 can reach: 1, 1/2, ... until alpha <= alpha_floor
inline int n_alpha_of(bool line_search, double alpha_floor) {
    int n = 1;
    if (line_search) { double a = 1.0; while (a > alpha_floor && n < 64) { a *= 0.5; n++; } }
    return n;
}

// Lanes per instance of k_backward_si_dpp, decided on the LAUNCHED (half-)batch: 16 while that gives every SIMD at most one wave (the launch is
// then bound by one wave's instruction stream, which is shorter with 4 instances per wave), 8 beyond (half the instructions per instance).
// Measured crossover between 4096 and 8192 instances on 1024 SIMDs.  Both groupings are bit-identical (test_sweep_lane_groupings_agree).
constexpr int si_lanes(int launched_B, int n_simd) { return (launched_B + 3) / 4 <= n_simd ? 16 : 8; }
// Workgroup form of k_backward_si_dpp (four waves = 16 consecutive instances per workgroup: the waves that share a 128-byte line of x, u on one
// CU), decided on the LAUNCHED (half-)batch, for the 16-lane grouping only: from this many instances on.  Both forms give the same bits
// (tests/test_gpu_sweep_wg.py), so the threshold is a pure speed choice.  Measured on C3 (profiles/sweep_wg_batch_scan.txt, ms per solve, lone
// waves against workgroups): B = 256 5.19 / 5.16, 1024 5.35 / 5.33, 2048 5.63 / 5.46, 3072 6.21 / 6.16, 4096 6.27 / 6.07 -- never slower at a
// measured size; smaller batches were not measured and stay on lone waves.
constexpr int SI_WG_MIN_BATCH = 256;
// The workgroup form with an I/O wave (a fifth wave that stores the gain records and the accepted x, u of the four chain waves, the latter as whole
// 128-byte lines, so that these stores leave the chains' instruction streams; 16 lanes per instance and at most one constraint row: two waves
// share a SIMD, 256 VGPRs), decided on the LAUNCHED (half-)batch: from this many instances on.  Same bits as the other forms
// (tests/test_gpu_sweep_io.py), so the threshold is a pure speed choice.  Measured on C3 (profiles/sweep_io_batch_scan.txt, ms per solve, four
// waves against four waves and the I/O wave): B = 256 5.14 / 5.07, 1024 5.31 / 5.25, 2048 5.45 / 5.40, 3072 6.13 / 6.02, 4096 6.09 / 5.98 -- never
// slower at a measured size; smaller batches were not measured and stay on lone waves, as for SI_WG_MIN_BATCH.  The halves of a split solve
// (ilqr_ctx_set_split(2)) were not measured either and keep the four-wave form under AUTO: the form's 99 KB of LDS allow one workgroup per CU, so
// two halves of 4096 instances on two streams could no longer share the CUs as the 20 KB workgroups of the four-wave form do.  The pin forces it there too.
// Since SI_PREP_MIN_BATCH (below) equals this threshold, AUTO never takes the I/O wave without the preparing waves; the pin SiWgIo still does.
constexpr int SI_IO_MIN_BATCH = 256;
constexpr bool si_io_supported(bool al, int m) { return !al || m <= 1; }
// The I/O-wave form with two preparing waves (they load xbar, ubar, x(1), u(1) and the multiplier, blend, form the limit terms and the AL
// bookkeeping and hand the chain waves what a step consumes through a ring in LDS: the chain waves load nothing in the loop but keypoint
// derivatives), wherever the I/O wave is taken and the LAUNCHED batch has this many instances.  Same bits (tests/test_gpu_sweep_prep.py), so the
// threshold is a pure speed choice.  Measured on C3 (profiles/sweep_prep_batch_scan.txt, ms per solve, the I/O-wave form against the same with the
// preparing waves): B = 256 5.08 / 4.63, 1024 5.27 / 4.81, 2048 5.40 / 4.96, 3072 6.07 / 5.65, 4096 5.96 / 5.56 -- faster at every measured size, so from
// the smallest one; smaller batches do not get the I/O wave.  148 KB of LDS: one workgroup per CU, as for the I/O-wave form; split halves keep the
// four-wave form under AUTO as there.  The pin forces it wherever the I/O wave is supported.
constexpr int SI_PREP_MIN_BATCH = 256;

// k_forward_reg with helper waves (a gain loader, an x | u loader and a storer per workgroup carry the loop's loads and line stores; the four
// chain waves keep the arithmetic: ilqr_kernels_wave.hip, ilqr_fwd_io_plan.hpp), wherever AUTO takes Forward::WaveWg on an unsplit solve and the
// LAUNCHED batch lies in [FWD_IO_MIN_BATCH, FWD_IO_MAX_BATCH].  Same bits (tests/test_gpu_forward_io.py), so the range is a pure speed choice.
// Measured on C3 (profiles/fwd_io_batch_scan.txt, ms per solve, ILQR_FWD=wg against wgio): B = 1024 5.18 / 5.06, 2048 5.27 / 5.15, 3072 5.36 / 5.24,
// 4096 5.54 / 5.45, 8192 9.83 / 9.87 -- faster from the smallest measured size up to 4096 instances, where 256 workgroups land on 256 CUs, and slower
// at 8192, where a CU runs a second round (71 KB of LDS per workgroup with packed records, 92 KB with plain ones: one workgroup per CU from 80 KB on).
// Nothing was measured between 4096 and 8192: the range ends at the largest size measured to win.  (AUTO takes Forward::WaveWg beyond 3072 instances
// only, so of this range it uses 3073 .. 4096; the rest matters where a later change moves that crossover.)  The halves of a split solve were not
// measured and keep the four-wave form.
constexpr int FWD_IO_MIN_BATCH = 1024;
constexpr int FWD_IO_MAX_BATCH = 4096;
constexpr bool fwd_io_auto(int launched_B) { return launched_B >= FWD_IO_MIN_BATCH && launched_B <= FWD_IO_MAX_BATCH; }

// Variant pins of ilqr_ctx_set_crosscheck: AUTO (0) = by batch size; the values are the ILQR_XC_* constants of include/ilqr_hip.h
enum class SweepPin { Auto = 0, Mfma = 1, Rows = 2, SiWave = 4, SiWg = 5, SiWgIo = 6, SiWgPrep = 7 };  // SiWave / SiWg / SiWgIo / SiWgPrep: the form of k_backward_si_dpp (same bits); AUTO elsewhere.  (3 is no pin: ilqr_ctx_set_crosscheck refuses it)
enum class FwdPin { Auto = 0, Wg = 1, Dpp = 2, WgLds = 3, WgIo = 4 };  // WgLds: Wg with k_forward_wg, the predecessor of k_forward_reg; WgIo: Wg with k_forward_reg's helper waves (same bits, all three)
enum class RerollPin { Auto = 0, Rows = 1, Dpp = 2 };

struct PlanIn {
    int kind = 0, nd = 1;
    bool al = false;
    int m = 0, per_step = 0;       // AL constraint rows (shared over k unless per_step)
    bool con_state_only = false;   // no constraint row touches the controls
    bool limits2_set = false;      // a second limit set (generic kernels only)
    bool shared_steps = false;     // keypoints that share a timestep (generic kernels only: the cooperative kernels hold one keypoint per step)
    bool obstacles = false;        // obstacle terms in the stage cost (generic kernels unless obstacles_coop: ilqr_obstacle.hpp)
    bool obstacles_coop = false;   // ilqr_ctx_set_obstacle_path(COOPERATIVE): such a problem may take the dense cooperative path (obs_coop_supported)
    bool uniform_R = false;        // all control weights equal
    bool off32 = true;             // x, u and the multipliers are addressable with 32-bit byte offsets (k_backward_si_dpp)
    bool line_search = true;
    double alpha_floor = 1e-3;
    int nb_iter = 0;
    int B = 0, n_simd = 1024;      // the whole batch; SIMDs of the device
    bool halves = false;           // the problem has split halves (B >= SPLIT_MIN_BATCH)
    int split = 1;                 // ilqr_ctx_set_split: 0 off, 1 where measured to pay, 2 every cooperative path
    bool profile = false;          // per-launch profiling: one stream, one kernel at a time
    bool generic = false;          // pin: the generic lane-per-instance kernels
    SweepPin sweep = SweepPin::Auto;
    FwdPin forward = FwdPin::Auto;
    RerollPin reroll = RerollPin::Auto;
};

enum class Init { Lti, Generic };                          // k_init_roll_lti + k_init_finish, or k_init_rollout
enum class Sweep { SiDpp, Mfma, Rows, Generic };           // k_backward_si_dpp, k_backward_mfma, k_backward_rows, k_backward (+ workspace)
enum class Forward { WaveWg, WaveDpp, Lin, Mfma, Generic };  // k_forward_reg (k_forward_wg if fwd_lds) / k_forward_dpp + k_select, k_forward_lin, k_forward_mfma + k_select_x, k_forward
enum class Apply {
    None,
    Wave,        // k_apply + k_flip_ran every iteration
    WaveLast,    // ... on the last iteration only: the next sweep applies the winner (fused)
    Lin,         // k_blend + k_flip
    RerollRows,  // k_apply_rows_tm: time systems, 8 lanes per instance through LDS
    RerollDpp,   // k_apply_dpp_tm: time systems, 16 lanes per instance on registers
};
constexpr int KD_SYM_KEEP = -1;  // no sweep runs: the gain records keep the layout of the last sweep that wrote them

struct RiccatiPlan {
    int n_alpha = 1;
    Init init = Init::Generic;
    bool init_al_update = false;  // k_al_post at it = -1 after the LTI rollout (active-set weights of the initial trajectory)
    Sweep sweep = Sweep::Generic;
    int si_lanes[2] = {16, 16};   // Sweep::SiDpp: lanes per instance of the whole batch or of each half (split)
    bool si_wg[2] = {false, false};  // Sweep::SiDpp with 16 lanes: the workgroup form (SI_WG_MIN_BATCH, or the pins SiWave / SiWg), per launched half
    bool si_prep[2] = {false, false};  // ... and the two preparing waves (SI_PREP_MIN_BATCH where AUTO takes the I/O wave, or the pin SiWgPrep; never under SiWave / SiWg / SiWgIo): only where si_io
    bool si_io[2] = {false, false};  // ... with the I/O wave (SI_IO_MIN_BATCH on an unsplit solve, or the pin SiWgIo; never under SiWave / SiWg): only where si_wg, at most one AL row
    Forward forward = Forward::Generic;
    bool fwd_lds = false;         // Forward::WaveWg under the pin FwdPin::WgLds: k_forward_wg instead of k_forward_reg
    bool fwd_io = false;          // Forward::WaveWg: k_forward_reg with its helper waves (fwd_io_auto on an unsplit solve, or the pin FwdPin::WgIo; never under Wg / WgLds)
    Apply apply = Apply::None;
    bool al_update = false;       // k_al_post after every line search (the wave path does it in k_apply or the fused sweep)
    bool fused = false;           // the sweep applies the previous line search's winner itself (ilqr_kernels_dpp.hip)
    int kd_sym = 0;               // layout the sweep writes: 1 packed symmetric (KD_SYM_RS), 0 plain, or KD_SYM_KEEP
    bool split = false;           // two halves on two streams
    bool needs_ws = false;        // the generic sweep keeps the matrices of a step in an explicit workspace
    bool obs_dense = false;       // obstacle terms on the cooperative kernels: dense stage derivatives (k_stage_dense) into k_backward_si_dpp<.., SW_DENSE>,
                                  // the obstacle cost of every step size (k_obs_ls) between the rollout and k_select, the accepted trajectory in memory
};

inline RiccatiPlan plan_riccati(const PlanIn& in) {
    RiccatiPlan p;
    const int kind = in.kind, nd = in.nd;
    p.n_alpha = n_alpha_of(in.line_search, in.alpha_floor);
    // Obstacle terms on the cooperative kernels (opt-in; the generic pin wins): not fused -- the accepted trajectory is in memory before the
    // derivative kernels read it (Apply::Wave) -- and on lone waves, since the workgroup, I/O-wave and preparing-wave forms are all fused.
    if (in.obstacles && in.obstacles_coop && !in.generic && !in.limits2_set && !in.shared_steps && in.off32 &&
        obs_coop_supported(kind, nd, in.al, in.m, in.per_step, in.con_state_only, p.n_alpha)) {
        p.obs_dense = true;
        p.init = Init::Lti;
        p.init_al_update = in.al;
        p.sweep = Sweep::SiDpp;
        p.si_lanes[0] = si_lanes(in.B, in.n_simd);
        p.si_lanes[1] = si_lanes(0, in.n_simd);
        const bool dpp = in.forward == FwdPin::Dpp || (in.forward == FwdPin::Auto && (in.B + 3) / 4 <= 3 * in.n_simd / 4);
        p.forward = dpp ? Forward::WaveDpp : Forward::WaveWg;
        p.fwd_lds = in.forward == FwdPin::WgLds;
        p.fwd_io = in.forward == FwdPin::WgIo;  // the pin only: the form was not measured on this path
        p.apply = Apply::Wave;
        p.kd_sym = in.nb_iter == 0 ? KD_SYM_KEEP : 0;
        return p;  // fused, al_update, split, needs_ws, si_wg, si_io, si_prep: false (fwd_io: by its pin alone)
    }
    // a second limit set, keypoints that share a timestep and obstacle terms exist in the generic kernels only, whatever the pins say
    const bool cooperative = !in.generic && !in.limits2_set && !in.shared_steps && !in.obstacles;
    const bool coop_fwd = cooperative && p.n_alpha <= 16;       // all step sizes at once (16 lanes / rows per instance)

    // sweep.  The row-per-lane sweep (16 lanes per instance, rows in registers): a lone wave's chain is longer than the matrix-core sweep's (553
    // against 316 us at the C4 shape), but four instances share a wave: it wins as soon as the wave-per-instance sweep needs a second round of
    // waves (measured: B = 2048 600 against 548 us, B = 4096 597 against 1040)
    if (cooperative && in.off32 && backward_si_supported(kind, nd, in.al, in.m, in.per_step, in.con_state_only)) p.sweep = Sweep::SiDpp;
    else if (cooperative && backward_mfma_supported(kind, nd, in.al, in.m)) {
        const bool pinned = in.sweep == SweepPin::Mfma || in.sweep == SweepPin::Rows;  // (SiWave / SiWg / SiWgIo / SiWgPrep pin nothing here)
        const bool rows = in.sweep == SweepPin::Rows || (!pinned && in.B > 2 * in.n_simd);
        p.sweep = rows && backward_rows_supported(kind, nd, in.al, in.m) ? Sweep::Rows : Sweep::Mfma;
    }

    // forward pass.  Single-integrator systems: small batches (up to three quarters of a wave of 4 instances per SIMD) roll out a chain, not a
    // stream -- k_forward_dpp.  Measured crossover with k_forward_wg on C3 (forward + decision, us): B = 2048 92 / 122, 3072 114 / 124, 4096 139 / 126
    if (coop_fwd && forward_wave_supported(kind, nd, p.n_alpha)) {
        const bool dpp = in.forward == FwdPin::Dpp || (in.forward == FwdPin::Auto && (in.B + 3) / 4 <= 3 * in.n_simd / 4);
        p.forward = dpp ? Forward::WaveDpp : Forward::WaveWg;
        p.fwd_lds = in.forward == FwdPin::WgLds;  // the large-batch pass at any batch size, as its predecessor wrote it
    } else if (coop_fwd && forward_lin_supported(kind, nd, p.n_alpha)) {
        p.forward = Forward::Lin;
    } else if (coop_fwd) {
        p.forward = Forward::Mfma;  // the time systems
    }
    const bool wave = p.forward == Forward::WaveWg || p.forward == Forward::WaveDpp;
    p.fused = p.sweep == Sweep::SiDpp && wave;
    // uniform control weights: the sweep's closed form for N = M D - I with D a multiple of I, writing the packed symmetric gain record
    // (ilqr_kernels.hpp: KD_SYM_RS) that the two forward passes of this path and the getters read; any other forward pass reads plain records
    p.kd_sym = in.nb_iter == 0 ? KD_SYM_KEEP : (p.fused && in.uniform_R) ? 1 : 0;

    // winner of the line search applied: the wave path in one pass with the AL bookkeeping and the buffer flip (or by the next sweep when fused);
    // k_forward_lin's cost pass writes no trajectory; the time systems re-roll the winner where the speculated step size lost -- 16 lanes per
    // instance on registers up to a quarter wave of 4 instances per SIMD (B = 256: 64 against 92 us), the 8-lanes-per-instance kernel beyond
    // (its waves cover 64 contiguous bytes of every [row][b] line, the other's 32: B = 2048 117 against 126 us, 4096 190 / 240)
    if (wave) p.apply = p.fused ? Apply::WaveLast : Apply::Wave;
    else if (p.forward == Forward::Lin) p.apply = Apply::Lin;
    else if (p.forward == Forward::Mfma && in.line_search) {
        const bool dpp = in.reroll == RerollPin::Dpp || (in.reroll == RerollPin::Auto && (in.B + 3) / 4 <= in.n_simd / 4);
        p.apply = dpp ? Apply::RerollDpp : Apply::RerollRows;
    }
    p.al_update = in.al && coop_fwd && !wave;

    p.init = cooperative && init_lti_supported(kind, nd) ? Init::Lti : Init::Generic;
    p.init_al_update = p.init == Init::Lti && in.al && !p.fused;

    // Two halves on two streams, the second one sweep behind (with per-launch profiling on, one stream: the event marks time one kernel at a time).
    // Measured (rocprofv3 kernel trace, B = 4096): it pays for the wave-per-instance MFMA sweep (C4: 60.3 -> 51.7 ms per solve; 4096 one-wave
    // workgroups on 3072 wave slots otherwise leave a one-third-full second round), not for the single-integrator pipeline (C3: the forward
    // pass slows from 0.125 to 0.24 ms and k_kp_derivs from 0.017 to 0.08-0.14 ms when they share the SIMDs with the other half's sweep:
    // 0.53 ms per iteration against 0.49 unsplit).
    p.split = coop_fwd && ((p.sweep == Sweep::Mfma && in.split) || in.split == 2) && !in.profile && in.halves && in.nb_iter > 0;
    p.needs_ws = p.sweep == Sweep::Generic && in.nb_iter > 0;
    // the helper-wave form of k_forward_reg: its pin, or AUTO on an unsplit solve in the measured range of launched batch sizes
    p.fwd_io = p.forward == Forward::WaveWg && !p.fwd_lds && (in.forward == FwdPin::WgIo || (in.forward == FwdPin::Auto && !p.split && fwd_io_auto(in.B)));
    const int b0 = p.split ? split_first_half(in.B) : in.B;
    p.si_lanes[0] = si_lanes(b0, in.n_simd);
    p.si_lanes[1] = si_lanes(in.B - b0, in.n_simd);
    // the 8-lane grouping (B > 4 n_simd) stays on the one-wave form, whatever the pin says
    const int launched[2] = {b0, in.B - b0};
    for (int h = 0; h < 2; h++) {
        const bool io_pin = in.sweep == SweepPin::SiWgIo || in.sweep == SweepPin::SiWgPrep;  // (SiWgPrep acts as SiWgIo where the preparing waves are not supported)
        const bool wg_pin = in.sweep == SweepPin::SiWg || io_pin;  // (SiWgIo acts as SiWg where the I/O wave is not supported)
        p.si_wg[h] = p.sweep == Sweep::SiDpp && p.si_lanes[h] == 16 && (wg_pin || (in.sweep != SweepPin::SiWave && launched[h] >= SI_WG_MIN_BATCH));
        p.si_io[h] = p.si_wg[h] && si_io_supported(in.al, in.m) &&
                     (io_pin || (in.sweep != SweepPin::SiWg && !p.split && launched[h] >= SI_IO_MIN_BATCH));
        p.si_prep[h] = p.si_io[h] && (in.sweep == SweepPin::SiWgPrep || (in.sweep != SweepPin::SiWgIo && launched[h] >= SI_PREP_MIN_BATCH));
    }
    return p;
}

}  // namespace ilqr
