// ilqr_kernels_dpp.hip -- closed-form backward Riccati sweep with the matrices in REGISTERS, rows broadcast by DPP (gfx950, fp64).
//
// Same mathematics as the cooperative sweep it replaces (reference: ILQRRecursive.cpp:68-97, AL-ILQR.cpp:110-145) for
// single-integrator dynamics (A = I, B = dt I):  S = Quu + reg I = D + dt^2 P,  M = S^-1,  N = M D - I,
//   K = N / dt,   d = -M Qu,   P' = l_xx - (D N + reg N'N) / dt^2,   p' = l_x + p - (Qu + D d)/dt - reg (D M d - d)/dt
// (exact consequences of (Quu + reg I) K = -Qux with the UN-regularised Quu in the value update, quirk D-3:
//  D - D M D = -D N and D M^2 D - D M - M D + I = N'N).
//
// Mapping.  The cooperative kernel gave every entry of the symmetric matrices a lane and moved the pivot column / row through LDS:
// one FMA per lane and pivot behind an LDS round trip.  Here LPI = 8 lanes own an instance (8 instances per wave), lane r of the
// group holds ROW r of every matrix (7 doubles; row 7 is padding and stays zero).  A pivot is
//     v_mov_b64_dpp  acc, s[c]  row_newbcast:c        the pivot element to all lanes of the DPP row
//     rc = 1/acc                                       (rcp + one cubic correction)
//     v_fmac_f64_dpp s[j], s[j], -t  row_newbcast:c    s[j] -= t * (pivot row)[j], t = s[c] rc, for the six j != c
// i.e. the broadcast of the pivot row is the DPP operand of the FMA itself: no LDS, no separate move, no wait.  A DPP row is 16
// lanes = two instances, so every broadcast instruction is issued twice, once per half with a bank mask (lanes 0-7 take lane c,
// lanes 8-15 take lane 8 + c); everything that is not a broadcast serves all eight instances with one instruction.  (LPI = 16 --
// one instance per DPP row, the second half a redundant copy -- needs one broadcast instruction but twice the waves; measured, see
// DESIGN.md.)  The products with M (N'N, M Qu, M d) are rows times broadcast rows in the same way.  No LDS at all; no barrier.
//
// Deferred row scaling.  The sweep operator turns the pivot row into a_cj / a_cc.  Scaling that one row would cost six multiplications
// executed for a single lane; instead row c keeps its values and remembers the factor (myrc): later pivots act on a row by
// row_i -= (a_ic rc') row_c', which commutes with a row scaling, so the stored row evolves exactly as the scaled one would, divided by
// its factor; the pivot element is stored as -1 and the multiplier of the pivot lane is 0 (the lane constants nz / nm1).  After the
// seven pivots the true row is myrc * stored = -(S^-1)_r.
//
// Hazards.  The compiler's hazard recogniser does not look inside inline assembly, so each pivot is ONE hand-ordered block: a DPP
// read of a VGPR needs two wait states after the VALU write (the block ends with two plain instructions after its last broadcast
// FMA, and inside it no instruction reads as DPP source what one of the two before it wrote); a transcendental result (v_rcp_f64)
// needs one (an independent multiplication follows the rcp).  Blocks whose DPP sources come straight from compiler-scheduled code
// start with s_nop 1.
//
// Addressing.  x / u live in the two halves of ONE allocation each (the problem allocates the double buffers back to back, with
// equal strides for X and U), so a 32-bit byte offset per lane and buffer serves every load and store of the loop with the
// uniform base in scalar registers; the host refuses batches whose arrays pass 4 GiB (they take the generic sweep).
//
// FUSED / AL bookkeeping exactly as before: the acceptance of the previous line search rides in the load path,
// x = xbar + alpha (x(1) - xbar) with k_apply's expression, I_k from the multipliers before the update, lambda update on update
// iterations, buffers flipped at the end (AL-ILQR.cpp:190, 202-208).
#include "../../include/ilqr_hip.h"
#include "ilqr_kernels.hpp"
#include "ilqr_lanes.hpp"
#include "ilqr_step.hpp"

namespace ilqr {

namespace {

#define DPPM_ALL " row_mask:0xf bank_mask:0xf"
#define DPPM_LO " row_mask:0xf bank_mask:0x3"
#define DPPM_HI " row_mask:0xf bank_mask:0xc"

// A DPP instruction reads its VGPR operands -- the broadcast source AND, for the lanes a bank mask leaves out, the old destination --
// ahead of the normal operand fetch: two wait states after any VALU write of one of them (found the hard way: a broadcast FMA
// right behind the `v_mov` that zeroed its accumulator gave wrong sums).  So every multi-instruction DPP sequence below is ONE asm
// statement that starts with `s_nop 1` (the compiler schedules freely around asm statements, never inside one), and inside a
// statement no instruction touches a register written by one of the two before it.

// acc[j] += sum_k bcast_k(src[j]) * mul[k]  for the seven j: row r of (lane rows of mul) x (matrix whose rows are the lanes' src)
template <int LPI>
__device__ __forceinline__ void fmac_rows_all(double (&acc)[7], const double (&src)[7], const double (&mul)[7]) {
#define R_(K, LL, MASK)                                                                                                                   \
    "v_fmac_f64_dpp %[a0], %[s0], %[m" #K "] row_newbcast:" LL MASK "\n\tv_fmac_f64_dpp %[a1], %[s1], %[m" #K "] row_newbcast:" LL MASK "\n\t" \
    "v_fmac_f64_dpp %[a2], %[s2], %[m" #K "] row_newbcast:" LL MASK "\n\tv_fmac_f64_dpp %[a3], %[s3], %[m" #K "] row_newbcast:" LL MASK "\n\t" \
    "v_fmac_f64_dpp %[a4], %[s4], %[m" #K "] row_newbcast:" LL MASK "\n\tv_fmac_f64_dpp %[a5], %[s5], %[m" #K "] row_newbcast:" LL MASK "\n\t" \
    "v_fmac_f64_dpp %[a6], %[s6], %[m" #K "] row_newbcast:" LL MASK "\n\t"
#define OPS_                                                                                                                              \
    : [a0] "+v"(acc[0]), [a1] "+v"(acc[1]), [a2] "+v"(acc[2]), [a3] "+v"(acc[3]), [a4] "+v"(acc[4]), [a5] "+v"(acc[5]), [a6] "+v"(acc[6])    \
    : [s0] "v"(src[0]), [s1] "v"(src[1]), [s2] "v"(src[2]), [s3] "v"(src[3]), [s4] "v"(src[4]), [s5] "v"(src[5]), [s6] "v"(src[6]),          \
      [m0] "v"(mul[0]), [m1] "v"(mul[1]), [m2] "v"(mul[2]), [m3] "v"(mul[3]), [m4] "v"(mul[4]), [m5] "v"(mul[5]), [m6] "v"(mul[6])
    if (LPI == 16)
        asm volatile("s_nop 1\n\t" R_(0, "0", DPPM_ALL) R_(1, "1", DPPM_ALL) R_(2, "2", DPPM_ALL) R_(3, "3", DPPM_ALL) R_(4, "4", DPPM_ALL) R_(5, "5", DPPM_ALL)
                         R_(6, "6", DPPM_ALL) "s_nop 0" OPS_);
    else
        asm volatile("s_nop 1\n\t" R_(0, "0", DPPM_LO) R_(0, "8", DPPM_HI) R_(1, "1", DPPM_LO) R_(1, "9", DPPM_HI) R_(2, "2", DPPM_LO) R_(2, "10", DPPM_HI)
                         R_(3, "3", DPPM_LO) R_(3, "11", DPPM_HI) R_(4, "4", DPPM_LO) R_(4, "12", DPPM_HI) R_(5, "5", DPPM_LO) R_(5, "13", DPPM_HI)
                             R_(6, "6", DPPM_LO) R_(6, "14", DPPM_HI) "s_nop 0" OPS_);
#undef R_
#undef OPS_
}
// sum_k bcast_k(src) * M[k]: three accumulators in rotation (no register is touched again within two instructions), zeroed inside
template <int LPI>
__device__ __forceinline__ double row_dot_bc(const double (&M)[7], double src) {
    double s0, s1, s2;
#define D_(A, K, LL, MASK) "v_fmac_f64_dpp %[" A "], %[x], %[m" #K "] row_newbcast:" LL MASK "\n\t"
#define OPS_                                                                                                                       \
    : [s0] "=&v"(s0), [s1] "=&v"(s1), [s2] "=&v"(s2)                                                                                \
    : [x] "v"(src), [m0] "v"(M[0]), [m1] "v"(M[1]), [m2] "v"(M[2]), [m3] "v"(M[3]), [m4] "v"(M[4]), [m5] "v"(M[5]), [m6] "v"(M[6])
#define ZERO_ "v_mov_b64 %[s0], 0\n\tv_mov_b64 %[s1], 0\n\tv_mov_b64 %[s2], 0\n\ts_nop 1\n\t"
    if (LPI == 16)
        asm volatile(ZERO_ D_("s0", 0, "0", DPPM_ALL) D_("s1", 1, "1", DPPM_ALL) D_("s2", 2, "2", DPPM_ALL) D_("s0", 3, "3", DPPM_ALL) D_("s1", 4, "4", DPPM_ALL)
                         D_("s2", 5, "5", DPPM_ALL) D_("s0", 6, "6", DPPM_ALL) "s_nop 0" OPS_);
    else
        // the same accumulator for a term in both halves (the sum's grouping must not depend on which half an instance sits in)
        asm volatile(ZERO_ D_("s0", 0, "0", DPPM_LO) D_("s1", 1, "1", DPPM_LO) D_("s2", 2, "2", DPPM_LO) D_("s0", 0, "8", DPPM_HI) D_("s1", 1, "9", DPPM_HI)
                         D_("s2", 2, "10", DPPM_HI) D_("s0", 3, "3", DPPM_LO) D_("s1", 4, "4", DPPM_LO) D_("s2", 5, "5", DPPM_LO) D_("s0", 3, "11", DPPM_HI)
                             D_("s1", 4, "12", DPPM_HI) D_("s2", 5, "13", DPPM_HI) D_("s0", 6, "6", DPPM_LO) "s_nop 1\n\t" D_("s0", 6, "14", DPPM_HI) "s_nop 0" OPS_);
#undef D_
#undef OPS_
#undef ZERO_
    return (s0 + s1) + s2;
}

// The seven pivots of the symmetric sweep with deferred row scaling as ONE hand-ordered block (see the header).  Pivot C:
//   acc = bcast_C(s[C]);  rc = 1/acc (v_rcp_f64 + cubic step);  t = (s[C] + s[C] nm1) rc  (nm1 = -1 in the pivot lane: t = 0 there);
//   s[j] -= t bcast_C(s[j]) (j != C);  s[C] = t + nm1 (-1 in the pivot lane);  myrc -= rc nm1 (the pivot lane remembers its factor)
// A DPP read needs two wait states after the write of its source: s[C+1] is last written by one of pivot C's FMAs, at least the two
// instructions of its tail ahead of pivot C+1's move; the rcp result is used one instruction later (an independent FMA between).
#define PV_HEAD16_(C) "v_mov_b64_dpp %[acc], %[s" #C "] row_newbcast:" #C DPPM_ALL "\n\t"
#define PV_HEAD8_(C, C8) "v_mov_b64_dpp %[acc], %[s" #C "] row_newbcast:" #C DPPM_LO "\n\tv_mov_b64_dpp %[acc], %[s" #C "] row_newbcast:" #C8 DPPM_HI "\n\t"
#define PV_RCP_(C)                                                                                                                \
    "v_rcp_f64 %[rc], %[acc]\n\t"                                                                                                 \
    "v_fma_f64 %[t], %[s" #C "], %[n" #C "], %[s" #C "]\n\t"                                                                      \
    "v_fma_f64 %[e], -%[acc], %[rc], 1.0\n\t"                                                                                     \
    "v_fma_f64 %[e], %[e], %[e], %[e]\n\t"                                                                                        \
    "v_fma_f64 %[rc], %[e], %[rc], %[rc]\n\t"                                                                                     \
    "v_mul_f64 %[t], %[t], %[rc]\n\t"
#define PV_F_(J, LL, MASK) "v_fmac_f64_dpp %[s" #J "], %[s" #J "], -%[t] row_newbcast:" LL MASK "\n\t"
#define PV_TAIL_(C) "v_add_f64 %[s" #C "], %[t], %[n" #C "]\n\tv_fma_f64 %[myrc], -%[rc], %[n" #C "], %[myrc]\n\t"
#define PV16_(C, A, B, D, E, F, G) PV_HEAD16_(C) PV_RCP_(C) PV_F_(A, #C, DPPM_ALL) PV_F_(B, #C, DPPM_ALL) PV_F_(D, #C, DPPM_ALL) PV_F_(E, #C, DPPM_ALL) PV_F_(F, #C, DPPM_ALL) PV_F_(G, #C, DPPM_ALL) PV_TAIL_(C)
#define PV8_(C, C8, A, B, D, E, F, G)                                                                                              \
    PV_HEAD8_(C, C8) PV_RCP_(C) PV_F_(A, #C, DPPM_LO) PV_F_(B, #C, DPPM_LO) PV_F_(D, #C, DPPM_LO) PV_F_(E, #C, DPPM_LO) PV_F_(F, #C, DPPM_LO) PV_F_(G, #C, DPPM_LO) \
        PV_F_(A, #C8, DPPM_HI) PV_F_(B, #C8, DPPM_HI) PV_F_(D, #C8, DPPM_HI) PV_F_(E, #C8, DPPM_HI) PV_F_(F, #C8, DPPM_HI) PV_F_(G, #C8, DPPM_HI) PV_TAIL_(C)
template <int LPI>
__device__ __forceinline__ void pivots(double (&s)[7], const double (&nm1)[7], double& myrc) {
    double acc, rc, e, t;
#define OPS_                                                                                                                              \
    : [acc] "=&v"(acc), [rc] "=&v"(rc), [e] "=&v"(e), [t] "=&v"(t), [s0] "+v"(s[0]), [s1] "+v"(s[1]), [s2] "+v"(s[2]), [s3] "+v"(s[3]),     \
      [s4] "+v"(s[4]), [s5] "+v"(s[5]), [s6] "+v"(s[6]), [myrc] "+v"(myrc)                                                                  \
    : [n0] "v"(nm1[0]), [n1] "v"(nm1[1]), [n2] "v"(nm1[2]), [n3] "v"(nm1[3]), [n4] "v"(nm1[4]), [n5] "v"(nm1[5]), [n6] "v"(nm1[6])
    if (LPI == 16)
        asm volatile("s_nop 1\n\t" PV16_(0, 1, 2, 3, 4, 5, 6) PV16_(1, 0, 2, 3, 4, 5, 6) PV16_(2, 0, 1, 3, 4, 5, 6) PV16_(3, 0, 1, 2, 4, 5, 6) PV16_(4, 0, 1, 2, 3, 5, 6)
                         PV16_(5, 0, 1, 2, 3, 4, 6) PV16_(6, 0, 1, 2, 3, 4, 5) "s_nop 0" OPS_);
    else
        asm volatile("s_nop 1\n\t" PV8_(0, 8, 1, 2, 3, 4, 5, 6) PV8_(1, 9, 0, 2, 3, 4, 5, 6) PV8_(2, 10, 0, 1, 3, 4, 5, 6) PV8_(3, 11, 0, 1, 2, 4, 5, 6)
                         PV8_(4, 12, 0, 1, 2, 3, 5, 6) PV8_(5, 13, 0, 1, 2, 3, 4, 6) PV8_(6, 14, 0, 1, 2, 3, 4, 5) "s_nop 0" OPS_);
#undef OPS_
}

// g = a_r . x - b over the eight lanes of an instance: product, tree and subtraction each rounded once
__device__ __forceinline__ double oct_row_g(double a_l, double x_l, double b) {
#pragma clang fp contract(off)
    const double p = a_l * x_l;
    return oct_sum_rounded(p) - b;
}

// (lds_addr, flag_read, flag_write and the bounded poll flag_wait_ge: ilqr_lanes.hpp)
// Bounded wait of a chain wave for the I/O wave's "consumed" word (LDS byte address `addr`, last read as `seen`) to reach `need`: at most
// SW_POLL_CHAIN polls; returns 1 if it gave up.
__device__ __forceinline__ int wait_consumed(int seen, unsigned addr, int need);
__device__ __forceinline__ double ldg(const double* base, unsigned byte_off) { return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(base) + byte_off); }
__device__ __forceinline__ void stg(double* base, unsigned byte_off, double v) { *reinterpret_cast<double*>(reinterpret_cast<char*>(base) + byte_off) = v; }

}  // namespace

// UNIF: every control weight is the same (R = r I, the common case): then N' = D M - I equals N = M D - I entry by entry
//
// WG: the workgroup form for large batches.  SW_WAVES = 4 waves with 16 consecutive instances per workgroup, so the four waves that share
// every 128-byte line of the [row][b] arrays (a wave of 4 instances touches 32 bytes of each of the 14 lines of a step, 28 when it loads)
// sit on ONE CU, as in k_forward_reg, instead of wherever the dispatcher puts four one-wave workgroups.  Nothing couples the waves: no
// barrier, no shared LDS, every wave runs the lone wave's code on its own image -- same bits (tests/test_gpu_sweep_wg.py).  Measured on C3
// at B = 4096 (profiles/sweep_wg_variations.txt): 6.09 against 6.30 ms per solve.  Staging the accepted x, u of a group of PF steps in an
// LDS block and storing full lines behind one barrier per group, as k_forward_reg does, was built and measured too: 6.37 ms -- the barrier
// costs a latency-bound chain 13 us per launch (6.11 with the barrier taken out, which is not a correct kernel), more than the lines save.
// 16 lanes per instance and the fused acceptance only.
//
// IO: the workgroup form with a fifth wave that executes no Riccati arithmetic and carries the stores of the four chain waves (bit 0: the
// gain records, bit 1: the accepted x, u as whole 128-byte lines: 16 instances x 8 bytes of one row).  A chain wave writes the gain image of
// its n-th step (n = 1 .. T - 1) into slot (n - 1) mod SW_RING of its ring in LDS, drops its blended x | u into the same slot of the
// workgroup's x | u ring (one ds_write per lane: the low half of an instance's 16 lanes holds x, the copy in the high half u) and then stores
// n into its word of sFl ("produced").  The I/O wave polls the four words; once every live chain wave has produced step n it reads the four
// images and the 14 x 16 block into registers, stores n into the workgroup's "consumed" word and sends the images where SEND_ sends them
// (the same 16-byte pieces, the same pst / kfull masks) and x, u as row segments, each lane under its own instance's blend and into its own
// instance's buffer.  A chain wave reads "consumed" at the start of the first step n of a group of PF steps and, at that step's end, needs
// consumed >= n + PF - SW_RING: that frees the slots of steps n .. n + PF, i.e. the group's images, its remaining x | u and the x | u of the
// next group's first step, which is written ahead of that group's check.  One check per group (a check per step cost the chain
// more than the stores it was relieved of: profiles/sweep_io_variations.txt).  Flags are plain LDS words written after the data they announce
// (a wave's LDS operations execute in order); one workgroup barrier before the loop (every wave has read active, pend and cur of the 16
// instances before a chain wave can finish and rewrite them), none inside.  Every wait is bounded (SW_POLL_CHAIN / SW_POLL_IO polls with
// s_sleep between them, more than 20 ms = a hundred launches): a wave that gives up clears `active` and sets ILQR_STATUS_SWEEP_IO on its
// instances and ends.  Two waves share a SIMD: at most 256 VGPRs, so not for MR = 4.  Same bits (tests/test_gpu_sweep_io.py).  Measured on C3
// at B = 4096 (profiles/sweep_io_ab_bench.txt): 5.99 against 6.08 ms per solve.
constexpr int SW_WAVES = 4;
constexpr int SW_RING = 8;             // slots per ring: two groups of PF steps, which lets the chain waves run 4 steps ahead of the I/O wave (with 4 slots: none)
constexpr int SW_POLL_CHAIN = 1 << 20; // polls of s_sleep 1 (64 clocks) + an LDS round trip: 28 ms at 2.4 GHz from the sleeps alone
constexpr int SW_POLL_IO = 1 << 18;    // polls of s_sleep 4 (256 clocks) + an LDS round trip: 28 ms at 2.4 GHz from the sleeps alone
// PREP (IO bit 2, with bits 0 and 1): two more waves that execute no Riccati arithmetic either and take everything of a step that depends only on
// what is loaded off the chain waves.  Preparing wave q serves chain waves 2 q and 2 q + 1 in the chain's own layout (lane j: row j mod 8 of instance
// 8 q + j / 8 of the workgroup, so the 8-lane butterfly of g = a . x - b is the chain's): it loads xbar, ubar, x(1), u(1) and the multiplier PF steps
// ahead, blends, drops x | u into the workgroup's x | u ring for the I/O wave, forms the limit terms and the AL bookkeeping (I_k, the multiplier
// update and its store) with the chain's expressions, writes {u, lim, l_x of the limits, I_k, lam + I_k g, beyond} of its (instance, row) into slot
// (n - 1) mod SW_PRING of the prepared ring and then stores n into its word of sFl ("prepared").  Before it writes step n it needs consumed >= n -
// SW_PRING: the I/O wave consumes a step only after every live chain wave has produced it, i.e. has read its prepared entry, so that one word frees
// both the prepared slot and the x | u slot.  A chain wave needs prepared >= the last step of a group of PF steps, checked once per group behind the
// pivots of the group's first step (which need nothing that is loaded); it loads nothing in the loop but the keypoint derivatives, does not blend
// and writes no x | u.  No cycle of waits: preparing step n waits for "consumed n - SW_PRING", that for "produced n - SW_PRING" of the chain waves,
// that for "prepared n - SW_PRING + PF - 1" at most -- always an earlier step.  Same bits (tests/test_gpu_sweep_prep.py).  Measured on C3
// at B = 4096 (profiles/sweep_prep_ab_bench.txt): 5.57 against 5.99 ms per solve; the chain wave's four-step loop went from 1768 to 1569 instructions.
constexpr int SW_PREP = 2;             // preparing waves: 8 instances each
constexpr int SW_PRING = 8;            // slots of the prepared ring = how far a preparing wave runs ahead of the I/O wave
constexpr int SW_PENT = 6;             // doubles per (instance, row) and slot: three 16-byte reads for the chain wave
namespace {
__device__ __forceinline__ int wait_consumed(int seen, unsigned addr, int need) { return flag_wait_ge(seen, addr, need, SW_POLL_CHAIN); }
}  // namespace
// DENSE (IO = SW_DENSE; lone waves, not fused: a problem with obstacle terms on the cooperative path, RiccatiPlan::obs_dense): EVERY step is a precomputed step.  l_x | l_xx
// of step k come from sw.sd[k] (k_stage_dense: the keypoint entry or the limit terms, plus the obstacle terms), in the element layout of a kpd entry;
// the keypoint and limit branches are never taken, the AL terms follow as they do otherwise.  The lane's eight doubles of a step (its row of l_xx and
// its component of l_x) ride in the same PF-steps-ahead ring as x, u and the multipliers: taken out at the top of the step, the slot's next loads
// issued right behind, so the chain never waits for a load issued in the same step.  64-bit addresses (sd is four times the size of X | U).
// The flag is bit 3 of IO (SW_DENSE), so that every other instantiation keeps its name: IOW below is what IO was.
template <int LPI, int MR, bool FUSED, bool UNIF, bool WG = false, int IO = 0>
__global__ __launch_bounds__(WG ? (SW_WAVES + ((IO & 7) ? 1 : 0) + ((IO & 4) ? SW_PREP : 0)) * 64 : 64) void k_backward_si_dpp(Bufs a, SweepArgs sw) {
    constexpr int IOW = IO & 7;              // the I/O wave's stages
    constexpr bool DENSE = (IO & 8) != 0;    // SW_DENSE
    constexpr int N = 7, IPW = 64 / LPI;
    static_assert(!DENSE || (!FUSED && !WG && IOW == 0), "the dense form: lone waves, the accepted trajectory in memory");
    constexpr int NWV = WG ? SW_WAVES : 1;
    constexpr bool IOK = (IOW & 1) != 0, IOX = (IOW & 2) != 0;  // the I/O wave sends the gain records / stores the accepted x, u
    constexpr bool PRP = (IOW & 4) != 0;                       // two preparing waves hand the chain waves what a step needs of x, u and the multipliers
    constexpr int NIMG = IOK ? SW_RING : 2, XRING = SW_RING, XROW = 18;
    static_assert(!PRP || (IOK && IOX && FUSED && SW_PRING == XRING && SW_WAVES * (64 / LPI) == 8 * SW_PREP), "the preparing waves: on top of the full I/O wave, one x | u slot per prepared slot");
    static_assert(!WG || (LPI == 16 && FUSED), "the workgroup form: 4 instances per wave, 16 per workgroup = one 128-byte line per row segment");
    static_assert(!IOW || (WG && MR <= 1), "the I/O wave: workgroup form, at most one constraint row (256 VGPRs at two waves on a SIMD)");
    constexpr int MRR = MR > 0 ? MR : 1;
    constexpr int ROWP = kd_rowp(N), RS = UNIF ? KD_SYM_RS : N * ROWP;  // uniform R: K is symmetric, the record holds its upper triangle (ilqr_kernels.hpp)
    static_assert(ROWP == 8, "a gain row is the lane's eight doubles {K_r0..K_r6, d_r}");
    static_assert(LPI == 8 || LPI == 16, "");
    // two images of the wave's gain records (written at the end of a step, sent out during the next) + one dump slot per lane behind each
    constexpr int NPQ_ = (IPW * (RS / 2) + 63) / 64, IMG = (IPW * RS > 128 * NPQ_) ? IPW * RS : 128 * NPQ_;
    __shared__ __attribute__((aligned(16))) double sKw[NWV][NIMG][IMG + 64];
    // IOX: the accepted x | u of a step, [row 0 .. 6 x, 7 .. 13 u, 14 dump][instance of the workgroup], row stride XROW (banks)
    __shared__ double sXU[IOX ? XRING : 1][IOX ? 2 * N + 1 : 1][IOX ? XROW : 1];
    // PRP: what the chain waves consume of a step, [slot][instance of the workgroup x 8 + row][u, lim, lx of the limits, I_k, lam + I_k g, beyond]
    __shared__ __attribute__((aligned(16))) double sPr[PRP ? SW_PRING : 1][PRP ? 8 * SW_WAVES * (64 / LPI) : 1][PRP ? SW_PENT : 2];
    __shared__ int sFl[IOW ? NWV + 1 + (PRP ? SW_PREP : 0) : 1];  // produced (per chain wave), consumed, prepared (per preparing wave)
    const DevDesc& d = *a.desc;
    const int wv = WG ? __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) : 0;
    double (*const sK)[IMG + 64] = sKw[wv < NWV ? wv : 0];
    const int lane = WG ? (int)threadIdx.x & 63 : (int)threadIdx.x, g = lane / LPI, l = lane % LPI;
    const int r = l & 7;                 // row of the matrices / component of the vectors this lane owns (7 = padding: all zeros)
    const bool low = l < 8;              // LPI = 16: the half that stores (the other half holds a second copy)
    const int b0 = (xcd_tile() * NWV + wv) * IPW;  // the wave's first instance
    const int b = b0 + g;
    const int Bp = d.Bp, T = d.T;
    const bool ok = (b < d.B) && a.active[b < d.B ? b : 0];
    const int bb = (b < d.B) ? b : 0;    // clamp so that every address stays valid; stores are guarded
    const int pendw = (FUSED && b < d.B) ? a.pend[bb] : 0;
    const bool acc = pendw > 0;
    if (IOW) {
        constexpr int RS_ = UNIF ? KD_SYM_RS : N * kd_rowp(N), PCS_ = RS_ / 2, NPQ2 = (IPW * PCS_ + 63) / 64;
        if (wv == NWV) {  // ---- the I/O wave: lane j looks at instance j mod 16 of the workgroup
            const int bi = xcd_tile() * (NWV * IPW) + (lane & 15);
            const bool in = bi < d.B;
            const int bbi = in ? bi : 0;
            const bool oki = in && a.active[bbi];
            const int pwi = in ? a.pend[bbi] : 0;
            const int curi = a.cur[bbi];
            __syncthreads();  // every wave has read active, pend and cur of the 16 instances; the flags are zero
            const unsigned okm16 = (unsigned)__ballot((oki && lane < 16) ? 1 : 0);
            const unsigned livem = (unsigned)__ballot(((oki || pwi > 0) && lane < 16) ? 1 : 0);  // the chain waves' early exit, per wave
            if (livem == 0u) return;
            bool live[NWV], kfull[NWV], pst[NWV][NPQ2];
            UNR for (int w = 0; w < NWV; w++) {
                live[w] = ((livem >> (w * IPW)) & 15u) != 0u;
                kfull[w] = ((okm16 >> (w * IPW)) & 15u) == 15u;
                UNR for (int q = 0; q < NPQ2; q++) {
                    const int c = lane + 64 * q, gi = (c / PCS_ < IPW) ? c / PCS_ : 0;
                    pst[w][q] = c < IPW * PCS_ && ((okm16 >> (w * IPW + gi)) & 1u);
                }
            }
            const bool want = (lane < NWV) ? ((livem >> (lane * IPW)) & 15u) != 0u : false;  // lane w polls chain wave w's word
            const int T1 = d.T - 1, Bpi = d.Bp;
            double* Ko = KD_REC(a.KD, Bpi, RS_, T1 - 1, xcd_tile() * (NWV * IPW));
            const ptrdiff_t Ks = (ptrdiff_t)Bpi * RS_;
            // accepted x, u: lane j stores rows (j / 16) + 4 q of instance j mod 16, into the buffer its x(1), u(1) were read from
            const bool blendi = pwi > 1;
            const unsigned bufoi = (unsigned)((a.X[1] - a.X[0]) * (ptrdiff_t)sizeof(double));
            const unsigned Vs = (unsigned)N * Bpi * 8u;
            unsigned oXi = (unsigned)(1 - curi) * bufoi + ((unsigned)((T1 - 1) * N) * Bpi + bbi) * 8u;
            for (int n = 1; n <= T1; n++) {
                for (int spins = 0;; spins++) {
                    const int pv = flag_read(&sFl[lane < NWV ? lane : 0]);
                    if (__ballot((want && pv < n) ? 1 : 0) == 0ull) break;
                    if (spins >= SW_POLL_IO) {  // a chain wave never produced step n: give up on the workgroup's instances
                        if (lane < 16 && in) { a.active[bbi] = 0; atomicOr(&a.status[bbi], ILQR_STATUS_SWEEP_IO); }
                        return;
                    }
                    __builtin_amdgcn_s_sleep(4);
                }
                LDS_ORDER();
                double kqa[NWV][NPQ2], kqb[NWV][NPQ2], xu[4];
                if (IOK) {
                    UNR for (int w = 0; w < NWV; w++) UNR for (int q = 0; q < NPQ2; q++) {
                        const double2 t2 = reinterpret_cast<const double2*>(sKw[w][(n - 1) % SW_RING])[lane + 64 * q];
                        kqa[w][q] = t2.x; kqb[w][q] = t2.y;
                    }
                }
                if (IOX) { UNR for (int q = 0; q < 4; q++) xu[q] = sXU[(n - 1) % XRING][(4 * q + (lane >> 4)) < 2 * N ? 4 * q + (lane >> 4) : 2 * N][lane & 15]; }
                flag_write(&sFl[NWV], n);  // consumed: the slots of step n are free
                if (IOK) {
                    UNR for (int w = 0; w < NWV; w++) {
                        if (!live[w]) continue;
                        double2* dst = reinterpret_cast<double2*>(Ko + w * (IPW * RS_)) + lane;
                        if (kfull[w]) {
                            UNR for (int q = 0; q + 1 < NPQ2; q++) dst[64 * q] = make_double2(kqa[w][q], kqb[w][q]);
                            if (lane + 64 * (NPQ2 - 1) < IPW * PCS_) dst[64 * (NPQ2 - 1)] = make_double2(kqa[w][NPQ2 - 1], kqb[w][NPQ2 - 1]);
                        } else {
                            UNR for (int q = 0; q < NPQ2; q++) if (pst[w][q]) dst[64 * q] = make_double2(kqa[w][q], kqb[w][q]);
                        }
                    }
                    Ko -= Ks;
                }
                if (IOX) {
                    if (blendi) {
                        UNR for (int q = 0; q < 4; q++) {
                            const int row = 4 * q + (lane >> 4);
                            if (row < N) stg(a.X[0], oXi + (unsigned)row * Bpi * 8u, xu[q]);
                            else if (row < 2 * N) stg(a.U[0], oXi + (unsigned)(row - N) * Bpi * 8u, xu[q]);
                        }
                    }
                    oXi -= Vs;
                }
            }
            return;
        }
        if (PRP && wv > NWV) {  // ---- a preparing wave: lane j owns row j mod 8 of instance 8 pw + j / 8 of the workgroup
            const int pw = wv - NWV - 1, iw = pw * 8 + (lane >> 3), rp = lane & 7;
            const int bi = xcd_tile() * (NWV * IPW) + iw;
            const bool in = bi < d.B;
            const int bbi = in ? bi : 0;
            const bool oki = in && a.active[bbi];
            const int pwi = in ? a.pend[bbi] : 0;
            const int curi = a.cur[bbi];
            __syncthreads();  // every wave has read active, pend and cur of the 16 instances; the flags are zero
            if (__ballot((oki || pwi > 0) ? 1 : 0) == 0ull) return;  // neither of its chain waves runs
            const bool acci = pwi > 0, blendi = pwi > 1;
            const double aacc = acci ? ldexp(1.0, -(pwi - 1)) : 1.0;
            int rd = curi, r1 = blendi ? 1 - curi : curi;
            if (acci && !blendi) rd = r1 = 1 - curi;
            const bool updi = acci && sw.do_update_prev;
            const bool isVp = rp < N;
            const int vp = isVp ? rp : 0;
            const int Bpp = d.Bp, Tp = d.T;
            const int lim_on = d.limits_set;
            const double pen = d.penalty, pen_xx = d.pen_xx;
            const int lw_v = isVp ? d.lw[vp] : 0;
            const double smax_v = lw_v != 0 ? d.smax[vp] : __builtin_inf(), smin_v = lw_v != 0 ? d.smin[vp] : -__builtin_inf();
            const double Avp = (MR == 1 && isVp) ? a.conA[vp] : 0.0, bp = (MR == 1) ? a.conb[0] : 0.0;
            double* const Xb = a.X[0];
            double* const Ub = a.U[0];
            const unsigned bufo = (unsigned)((a.X[1] - a.X[0]) * (ptrdiff_t)sizeof(double));
            const unsigned Vstep = (unsigned)N * Bpp * 8u, Lstep = (unsigned)MR * Bpp * 8u;
            unsigned oA = (unsigned)rd * bufo + ((unsigned)((Tp - 2) * N + vp) * Bpp + bbi) * 8u;  // xbar, ubar
            unsigned oB = (unsigned)r1 * bufo + ((unsigned)((Tp - 2) * N + vp) * Bpp + bbi) * 8u;  // x(1), u(1)
            unsigned oL = ((unsigned)(Tp - 2) * MR * Bpp + bbi) * 8u, oLw = oL;                   // the multiplier: loads, store
            constexpr int PF = 4;
            double xr[PF], ur[PF], x1r[PF], u1r[PF], lr[PF];
            auto fetch = [&](int slot, int kk) {  // as the chain waves' fetch: every load unconditional
                xr[slot] = ldg(Xb, oA);
                ur[slot] = ldg(Ub, oA);
                x1r[slot] = ldg(Xb, oB);
                u1r[slot] = ldg(Ub, oB);
                lr[slot] = 0;
                if (MR > 0) lr[slot] = ldg(a.lambda, oL);
                if (kk > 0) { oA -= Vstep; oB -= Vstep; oL -= Lstep; }
            };
            UNR for (int q = 0; q < PF; q++) { fetch(q, Tp - 2 - q); __builtin_amdgcn_sched_barrier(0); }
            const unsigned fl_c = lds_addr(&sFl[NWV]);
            int gave = 0;  // uniform
            for (int k0 = Tp - 2; k0 >= 0; k0 -= PF) {
              const int s0 = (Tp - 2 - k0) % SW_PRING;  // uniform: the slot of the group's first step
              UNR for (int jj = 0; jj < PF; jj++) {
                const int k = k0 - jj;
                double xv = ring_take(xr[jj]), uv = ring_take(ur[jj]);
                const double x1v = ring_take(x1r[jj]), u1v = ring_take(u1r[jj]);
                xv = fma(aacc, x1v - xv, xv);  // accepted trajectory (k_apply's expression)
                uv = fma(aacc, u1v - uv, uv);
                double lam = (MR > 0) ? ring_take(lr[jj]) : 0.0;
                __builtin_amdgcn_sched_barrier(0);
                fetch(jj, k - PF);
                if (k < 0) continue;  // uniform: dummy step of the last group
                // step n = T - 1 - k goes into the slots of step n - SW_PRING: free once the I/O wave has consumed that step (one asm statement, as in the chain waves)
                const int need = __builtin_amdgcn_readfirstlane(Tp - 1 - k - SW_PRING);
                gave |= wait_consumed(flag_read(&sFl[NWV]), fl_c, need);
                sXU[s0 + jj][isVp ? vp : 2 * N][iw] = xv;  // the I/O wave stores them as lines, under the instance's own blend
                sXU[s0 + jj][isVp ? N + vp : 2 * N][iw] = uv;
                double beyond = 0, lim = 0, lxl = 0, Isk = 0, lt = 0;
                if (lim_on) {  // uniform.  The chain waves' expressions
                    beyond = fmax(xv - smax_v, 0.0) + fmax(smin_v - xv, 0.0);
                    lim = (beyond > 0.0) ? pen_xx : 0.0;
                    lxl = pen * fmax(xv - smax_v, 0.0) - pen * fmax(smin_v - xv, 0.0);
                }
                if (MR == 1) {
                    const double gr = oct_row_g(Avp, xv, bp);
                    Isk = sw.pen_in * ((gr < 0 && lam == 0) ? 0.0 : 1.0);
                    const double nv = fma(sw.pen_update_prev, gr, lam);
                    const double nl = nv > 0 ? nv : 0;
                    lam = updi ? nl : lam;
                    if (updi && rp == 0) stg(a.lambda, oLw, lam);
                    lt = lam + Isk * gr;
                    oLw -= Lstep;
                }
                double2* e = reinterpret_cast<double2*>(sPr[s0 + jj][iw * 8 + rp]);
                e[0] = make_double2(uv, lim);
                e[1] = make_double2(lxl, Isk);
                e[2] = make_double2(lt, beyond);
                flag_write(&sFl[NWV + 1 + pw], Tp - 1 - k);  // prepared: after the data it announces
              }
              k0 = gave ? 0 : k0;  // (a select on the loop counter, no branch: the loop ends here)
            }
            if (gave && rp == 0 && in) { a.active[bbi] = 0; atomicOr(&a.status[bbi], ILQR_STATUS_SWEEP_IO); }  // the I/O wave is gone
            return;
        }
        if (lane == 0) { sFl[wv] = 0; if (wv == 0) { sFl[NWV] = 0; if (PRP) { UNR for (int q = 0; q < SW_PREP; q++) sFl[NWV + 1 + q] = 0; } } }
        __syncthreads();
    }
    if (__ballot((ok || acc) ? 1 : 0) == 0ull) return;  // wave-uniform (the waves of a workgroup never meet in the loop)

    const bool isV = r < N;
    const int v = isV ? r : 0;
    const int cur = a.cur[bb];
    // the two buffers of X (of U) are the halves of one allocation with the same stride for X and U
    double* const Xb = a.X[0];
    double* const Ub = a.U[0];
    const unsigned bufo = (unsigned)((a.X[1] - a.X[0]) * (ptrdiff_t)sizeof(double));
    const double aacc = acc ? ldexp(1.0, -(pendw - 1)) : 1.0;
    const bool blend = acc && pendw > 1;  // alpha = 1: the other buffer already holds the accepted trajectory
    // xbar / ubar are read from buffer `rd`, x(1) / u(1) from buffer `r1`, and the accepted x, u are written over x(1), u(1).  Without a
    // pending acceptance both read xbar (x(1) - xbar = 0 reproduces xbar exactly) and nothing is stored.
    int rd = cur, r1 = blend ? 1 - cur : cur;
    if (FUSED && acc && !blend) rd = r1 = 1 - cur;
    const bool upd = FUSED && acc && sw.do_update_prev;
    const bool wr = blend && isV && low;  // this lane stores the accepted x, u
    const double dt = d.dt, idt = 1.0 / dt, idt2 = idt * idt, reg = d.reg, dt2 = dt * dt;
    const double Rv = isV ? d.R_diag[v] : 0.0, Dv = isV ? Rv + reg : 0.0;
    const int lim_on = d.limits_set;
    const double pen = d.penalty, pen_xx = d.pen_xx;
    const int lw_v = isV ? d.lw[v] : 0;
    // bounds with the weight folded in: an unweighted coordinate gets (+inf, -inf), which no x violates (a NaN neither)
    const double smax_v = lw_v != 0 ? d.smax[v] : __builtin_inf(), smin_v = lw_v != 0 ? d.smin[v] : -__builtin_inf();

    // lane constants: nm1[c] = -1 in the lane whose row is the pivot row of pivot c, 0 elsewhere
    double nm1[N], Dd[N], Dj[N];
    UNR for (int c = 0; c < N; c++) {
        nm1[c] = (r == c) ? -1.0 : 0.0;
        Dj[c] = d.R_diag[c] + reg;       // wave-uniform
        Dd[c] = (r == c) ? Dj[c] : 0.0;  // row r of D
    }
    const double cDN = Dv * idt2, cRN = reg * idt2;
    // constraint rows (state part only: checked on the host)
    const int m = (MR == 1) ? 1 : a.m;
    double Av[MRR], bbr[MRR], Arow[MRR][N];
    UNR for (int rr = 0; rr < MRR; rr++) {
        Av[rr] = bbr[rr] = 0;
        UNR for (int q = 0; q < N; q++) Arow[rr][q] = 0;
        if (MR > 0 && rr < m) {
            const double* Ar = a.conA + (size_t)rr * 2 * N;
            Av[rr] = isV ? Ar[v] : 0.0;
            bbr[rr] = a.conb[rr];
            UNR for (int q = 0; q < N; q++) Arow[rr][q] = Ar[q];
        }
    }
    // byte offsets (32 bit) of the lane's element at the step being loaded, one step = Vstep bytes back
    const unsigned Vstep = (unsigned)N * Bp * 8u, Lstep = (unsigned)m * Bp * 8u;
    unsigned oA = (unsigned)rd * bufo + ((unsigned)((T - 2) * N + v) * Bp + bb) * 8u;  // xbar, ubar
    unsigned oB = (unsigned)r1 * bufo + ((unsigned)((T - 2) * N + v) * Bp + bb) * 8u;  // x(1), u(1)
    unsigned oL = ((unsigned)(T - 2) * m * Bp + bb) * 8u;                              // multipliers / I_k of row 0
    // gain records of the wave's instances (adjacent in memory): 16-byte pieces, piece c of the image belongs to instance c / (RS / 2)
    constexpr int PCS = RS / 2, NPQ = (IPW * PCS + 63) / 64;
    const unsigned long long okm = __ballot(ok ? 1 : 0);
    bool pst[NPQ];
    const bool kfull = okm == ~0ull;  // every instance of the wave stores its gains: only the ragged tail of the last round is masked
    UNR for (int q = 0; q < NPQ; q++) {
        const int c = lane + 64 * q, gi = (c / PCS < IPW) ? c / PCS : 0;
        pst[q] = c < IPW * PCS && ((okm >> (gi * LPI)) & 1ull);
    }
    // where this lane's entries go in the image (doubles): uniform R -- the upper triangle of its row and d_r, the rest to the lane's dump slot
    int wo[N], wod = IMG + lane;
    UNR for (int j = 0; j < N; j++) wo[j] = IMG + lane;
    if (UNIF) {
        if (isV && low) {
            UNR for (int j = 0; j < N; j++) wo[j] = (j >= v) ? g * RS + kd_sym_tri(v, j) : IMG + lane;
            wod = g * RS + KD_SYM_D + v;
        }
        if (l == 0) { UNR for (int i = 0; i < NIMG; i++) sK[i][g * RS + KD_SYM_RS - 1] = 0; }  // the pad entry of the record
    }
    double* Kout = KD_REC(a.KD, Bp, RS, T - 2, b0);  // (the gains of a big batch pass 4 GiB: 64-bit pointer)
    const ptrdiff_t Kstep = (ptrdiff_t)Bp * RS;

    int kpi = d.n_kp - 1;
    int kp_next = (kpi >= 0) ? d.kp_t[kpi] : -1;
    const size_t kpd_stride = (size_t)(N + N * N) * Bp;

    // terminal values: P = l_xx(x_{T-1}), p = l_x(x_{T-1})
    double P[N], p = 0;
    UNR for (int j = 0; j < N; j++) P[j] = 0;
    {
        double xv = ldg(Xb, oA + Vstep);
        if (FUSED) {
            const double x1 = ldg(Xb, oB + Vstep);
            xv = fma(aacc, x1 - xv, xv);
            if (wr) stg(Xb, oB + Vstep, xv);
        }
        if (DENSE) {
            const double* src = sw.sd + (size_t)(T - 1) * kpd_stride;
            if (isV) {
                UNR for (int j = 0; j < N; j++) P[j] = AT(src, N + v * N + j, bb);
                p = AT(src, v, bb);
            }
        } else if (kp_next == T - 1) {
            const double* src = a.kpd + (size_t)kpi * kpd_stride;
            if (isV) {
                UNR for (int j = 0; j < N; j++) P[j] = AT(src, N + v * N + j, bb);
                p = AT(src, v, bb);
            }
            kpi--;
            kp_next = (kpi >= 0) ? d.kp_t[kpi] : -1;
        } else if (lim_on) {
            const double beyond = fmax(xv - smax_v, 0.0) + fmax(smin_v - xv, 0.0);
            const double lim = (beyond > 0.0) ? pen_xx : 0.0;
            UNR for (int j = 0; j < N; j++) P[j] = -nm1[j] * lim;
            if (lw_v != 0) {
                if (xv > smax_v) p = -pen * (smax_v - xv);
                else if (xv < smin_v) p = -pen * (smin_v - xv);
            }
        }
    }
    // PF-steps-ahead prefetch ring (vmcnt retires in issue order: a load issued one step ahead would wait for the previous step's stores)
    constexpr int PF = 4;
    double xr[PF], ur[PF], x1r[PF], u1r[PF], lr[PF][MRR], ir[PF][MRR];
    constexpr int ND = DENSE ? N + 1 : 1;
    double dr[PF][ND];  // DENSE: the lane's row of l_xx and its component of l_x
    const size_t sd_row = (size_t)Bp;
    const double* sdm = DENSE ? sw.sd + (size_t)(T - 2) * kpd_stride + (size_t)(N + v * N) * Bp + bb : nullptr;  // row v of l_xx of the step being loaded
    const double* sdx = DENSE ? sw.sd + (size_t)(T - 2) * kpd_stride + (size_t)v * Bp + bb : nullptr;            // component v of l_x
    unsigned rofs[MRR];
    UNR for (int rr = 0; rr < MRR; rr++) rofs[rr] = (unsigned)((MR > 0 && rr < m) ? rr : 0) * Bp * 8u;
    auto fetch = [&](int slot, int kk) {  // loads of timestep max(kk, 0) into ring slot; every load unconditional (a CFG path that skips
        xr[slot] = ldg(Xb, oA);           // one makes the waitcnt pass fall back to vmcnt(0))
        ur[slot] = ldg(Ub, oA);
        x1r[slot] = u1r[slot] = 0;
        if (FUSED) { x1r[slot] = ldg(Xb, oB); u1r[slot] = ldg(Ub, oB); }
        UNR for (int rr = 0; rr < MRR; rr++) {
            lr[slot][rr] = ir[slot][rr] = 0;
            if (MR > 0) { lr[slot][rr] = ldg(a.lambda, oL + rofs[rr]); if (!FUSED) ir[slot][rr] = ldg(a.Is, oL + rofs[rr]); }
        }
        if (DENSE) {
            UNR for (int j = 0; j < N; j++) dr[slot][j] = sdm[(size_t)j * sd_row];
            dr[slot][ND - 1] = sdx[0];
            if (kk > 0) { sdm -= kpd_stride; sdx -= kpd_stride; }
        }
        if (kk > 0) { oA -= Vstep; oB -= Vstep; oL -= Lstep; }  // uniform; no load inside the branch
    };
    if (!PRP) { UNR for (int q = 0; q < PF; q++) { fetch(q, T - 2 - q); __builtin_amdgcn_sched_barrier(0); } }
    // store side of the fused acceptance: the accepted x, u of step k go where x(1), u(1) were read (PF steps behind the loads)
    unsigned oW = (unsigned)r1 * bufo + ((unsigned)((T - 2) * N + v) * Bp + bb) * 8u;
    unsigned oLw = ((unsigned)(T - 2) * m * Bp + bb) * 8u;

    static_assert(SW_RING % PF == 0, "a step's slot is the group's first slot + its place in the group");
    const unsigned fl_cons = lds_addr(&sFl[IOW ? NWV : 0]);
    const int fl_pi = PRP ? NWV + 1 + wv / (SW_WAVES / SW_PREP) : 0;  // PRP: the wave's preparing wave
    const unsigned fl_prep = lds_addr(&sFl[fl_pi]);
    const int pent = (wv * IPW + g) * 8 + r;                             // PRP: the lane's entry of a prepared slot (both halves of an instance read the same)
    int gave_up = 0;  // uniform
    const int xcol = wv * IPW + g, xrow = isV ? (low ? v : N + v) : 2 * N;  // IOX: where this lane drops its x (low half) or u (the copy)
    for (int k0 = T - 2; k0 >= 0; k0 -= PF) {
      const int sl0 = IOK ? (T - 2 - k0) % SW_RING : 0, xs0 = IOX ? (T - 2 - k0) % XRING : 0;  // uniform: the slots of the group's first step
      UNR for (int jj = 0; jj < PF; jj++) {
        const int k = k0 - jj;
        double xv = 0, uv = 0;
        if (!PRP) { xv = ring_take(xr[jj]); uv = ring_take(ur[jj]); }
        if (FUSED && !PRP) {  // accepted trajectory (k_apply's expression)
            const double x1v = ring_take(x1r[jj]), u1v = ring_take(u1r[jj]);
            xv = fma(aacc, x1v - xv, xv);
            uv = fma(aacc, u1v - uv, uv);
        }
        double lam[MRR], Isk[MRR];
        UNR for (int rr = 0; rr < MRR; rr++) {
            lam[rr] = (MR > 0 && !PRP) ? ring_take(lr[jj][rr]) : 0.0;
            Isk[rr] = PRP ? 0.0 : (MR > 0 && !FUSED) ? ring_take(ir[jj][rr]) : ir[jj][rr];
        }
        double dlxx[N], dlx = 0;
        UNR for (int j = 0; j < N; j++) dlxx[j] = DENSE ? ring_take(dr[jj][j]) : 0.0;
        if (DENSE) dlx = ring_take(dr[jj][ND - 1]);
        if (!PRP) {
            __builtin_amdgcn_sched_barrier(0);  // the slots are free: only now their next loads
            fetch(jj, k - PF);
        }
        const int prepared = (PRP && jj == 0) ? flag_read(&sFl[fl_pi]) : 0;       // read here, needed behind the pivots
        const int consumed = (IOW && jj == 0) ? flag_read(&sFl[IOW ? NWV : 0]) : 0;  // read here, needed at the step's end
        // the image of the step before this one (in time) leaves now: LDS -> registers here, registers -> memory after the pivots
        const bool kprev = k < T - 2;
        double kqa[NPQ], kqb[NPQ];  // (two arrays of doubles: an array of double2 -- or anything a lambda captures by reference -- goes to scratch)
        if (!IOK) {
            UNR for (int q = 0; q < NPQ; q++) {  // unconditional: stays inside the (padded) array
                const double2 t2 = reinterpret_cast<const double2*>(sK[(jj + 1) & 1])[lane + 64 * q];
                kqa[q] = t2.x; kqb[q] = t2.y;
            }
        }
#define SEND_()                                                                                                         \
        {                                                                                                               \
            double2* dst = reinterpret_cast<double2*>(Kout + Kstep) + lane;                                             \
            if (kfull) {                                                                                                \
                UNR for (int q = 0; q + 1 < NPQ; q++) dst[64 * q] = make_double2(kqa[q], kqb[q]);                       \
                if (lane + 64 * (NPQ - 1) < IPW * PCS) dst[64 * (NPQ - 1)] = make_double2(kqa[NPQ - 1], kqb[NPQ - 1]);  \
            } else {                                                                                                    \
                UNR for (int q = 0; q < NPQ; q++) if (pst[q]) dst[64 * q] = make_double2(kqa[q], kqb[q]);               \
            }                                                                                                           \
        }
        if (k < 0) {  // uniform: dummy step of the last group; the one right behind the last real step sends its image out
            if (!IOK && k == -1) SEND_()
            continue;
        }
        // PRP: the step's prepared entry {u, lim | lx of the limits, I_k | lam + I_k g, beyond}; the group's check stands behind the first step's pivots
        double2 pe0 = make_double2(0, 0), pe1 = pe0, pe2 = pe0;
#define PREP_READ_()                                                                          \
        {                                                                                     \
            const double2* e = reinterpret_cast<const double2*>(sPr[PRP ? sl0 + jj : 0][PRP ? pent : 0]); \
            pe0 = e[0]; pe1 = e[1]; pe2 = e[2];                                               \
        }
        if (PRP && jj > 0) PREP_READ_()
        if (FUSED && !PRP) {
            if (IOX) sXU[xs0 + jj][xrow][xcol] = low ? xv : uv;  // the I/O wave stores them as lines, under the instance's own blend
            else if (wr) { stg(Xb, oW, xv); stg(Ub, oW, uv); }
            oW -= Vstep;
        }
        const double Qu0 = PRP ? 0.0 : Rv * uv + dt * p;  // Qu = R u + B'p
        // ---- S = D + dt^2 P (row r), then the seven pivots: afterwards myrc * s = row r of -S^-1
        double s[N];
        UNR for (int j = 0; j < N; j++) s[j] = fma(dt2, P[j], Dd[j]);
        double myrc = 0.0;
        pivots<LPI>(s, nm1, myrc);
        if (!IOK && kprev) SEND_()
        if (PRP && jj == 0) {  // once per group: its last step (of the sweep: T - 1) is prepared.  The bounded poll falls through at once in the common case
            const int last = T - 1 - k + PF - 1;
            gave_up |= wait_consumed(prepared, fl_prep, __builtin_amdgcn_readfirstlane(last < T - 1 ? last : T - 1));
            PREP_READ_()
        }
        const double Qu = PRP ? Rv * pe0.x + dt * p : Qu0;
        const double nrc = -myrc;
        // row r of S^-1 is M = nrc s.  With uniform control weights M is never formed: N = M D - I = (nrc D) s - I, and the two
        // products with M run on s and are scaled afterwards.
        double M[N], Nn[N], ntc[N], Kr[N];
        if (UNIF) {
            const double nrcD = nrc * Dj[0];
            UNR for (int j = 0; j < N; j++) {
                Nn[j] = fma(s[j], nrcD, nm1[j]);  // row r of N = M D - I (= row r of N' = D M - I)
                ntc[j] = Nn[j] * -cRN;
                Kr[j] = Nn[j] * idt;              // K = N / dt
            }
        } else {
            UNR for (int j = 0; j < N; j++) {
                M[j] = nrc * s[j];
                Nn[j] = fma(M[j], Dj[j], nm1[j]);
                ntc[j] = fma(Dv, M[j], nm1[j]) * -cRN;  // -reg/dt^2 x row r of N' = D M - I (M symmetric)
                Kr[j] = Nn[j] * idt;
            }
        }
        // ---- d = -M Qu
        const double dv = UNIF ? myrc * row_dot_bc<LPI>(s, Qu) : -row_dot_bc<LPI>(M, Qu);
        // ---- gains out.  The lane's row {K_r0 .. K_r6, d_r} is 64 contiguous bytes of the record, but stored from here a store
        // instruction would write 16-byte pieces 64 bytes apart: 56 partial-sector writes per instruction, which at four waves per CU
        // doubled the launch (measured: 381 -> 194 us at B = 8192 with these stores removed).  The rows go into a wave-local LDS image of
        // the wave's records as they lie in memory; the image leaves during the NEXT step as 16-byte pieces of whole lines (1 KiB
        // contiguous per instruction), so neither the LDS round trip nor the stores sit on this step's chain.
        if (IOW && jj == 0) {  // once per group of PF steps n .. n + PF - 1 (n = T - 1 - k), behind the x | u write of step n and ahead of every other
            // write of the group and of the x | u write of step n + PF, which opens the next group ahead of that group's check: the last of these
            // slots, step n + PF's, is free once step n + PF - SW_RING is consumed (the x | u slot of step n itself was covered by the check of
            // the group before, or is the ring's first use).
            // No branch for the compiler to see: the bounded poll is one asm statement that falls through at once in the common case, and
            // a wave that gave up finishes this group on slots it may not own and then leaves the loop (below).
            const int need = __builtin_amdgcn_readfirstlane(T - 1 - k + PF - SW_RING);
            gave_up |= wait_consumed(consumed, fl_cons, need);
        }
        if (UNIF) {  // packed symmetric record: row r contributes K_rr .. K_r6 and d_r; everything else (and every lane without a row) writes its dump slot -- no mask
            double* img = sK[IOK ? sl0 + jj : jj & 1];
            UNR for (int j = 0; j < N; j++) img[wo[j]] = Kr[j];
            img[wod] = dv;
        } else if (isV && low) {
            double2* w = reinterpret_cast<double2*>(&sK[IOK ? sl0 + jj : jj & 1][g * RS + v * ROWP]);
            w[0] = make_double2(Kr[0], Kr[1]);
            w[1] = make_double2(Kr[2], Kr[3]);
            w[2] = make_double2(Kr[4], Kr[5]);
            w[3] = make_double2(Kr[6], dv);
        }
        if (IOW) flag_write(&sFl[wv], T - 1 - k);  // produced: after the data it announces
        Kout -= Kstep;
        // ---- stage derivatives l_xx (row r), l_x (component r), accumulated onto -D N / dt^2
        double Pn[N], lx = 0;
        UNR for (int j = 0; j < N; j++) Pn[j] = -cDN * Nn[j];
        if (DENSE) {  // every step precomputed (k_stage_dense); the loads were consumed at the top of the step
            if (isV) { UNR for (int j = 0; j < N; j++) Pn[j] += dlxx[j]; lx = dlx; }
        } else if (k == kp_next) {  // uniform: keypoint step, precomputed by k_kp_derivs (incl. limits)
            const double* src = a.kpd + (size_t)kpi * kpd_stride;
            double lxx[N];
            UNR for (int j = 0; j < N; j++) lxx[j] = AT(src, N + v * N + j, bb);
            lx = AT(src, v, bb);
            if (!isV) { UNR for (int j = 0; j < N; j++) lxx[j] = 0; lx = 0; }
            UNR for (int j = 0; j < N; j++) Pn[j] += lxx[j];
            // consume the loads inside the branch: otherwise their wait lands after the join and every step drains vmcnt to 0
            UNR for (int j = 0; j < N; j++) asm volatile("" : "+v"(Pn[j]));
            asm volatile("" : "+v"(lx));
            kpi--;
            kp_next = (kpi >= 0) ? __builtin_amdgcn_readfirstlane(d.kp_t[kpi]) : -1;
        } else if (PRP && lim_on) {  // uniform.  The preparing wave's beyond, lim and l_x
            const double lim = pe0.y;
            if (__ballot(pe2.y > 0.0 ? 1 : 0) != 0ull) { UNR for (int j = 0; j < N; j++) Pn[j] = fma(-nm1[j], lim, Pn[j]); }  // uniform; adds exact zeros otherwise
            lx = pe1.x;
        } else if (lim_on) {  // uniform.  inspectJointLimit (System.cpp:121-142) branch-free; l_xx of the limits is diagonal
            const double beyond = fmax(xv - smax_v, 0.0) + fmax(smin_v - xv, 0.0);
            const double lim = (beyond > 0.0) ? pen_xx : 0.0;
            if (__ballot(beyond > 0.0 ? 1 : 0) != 0ull) { UNR for (int j = 0; j < N; j++) Pn[j] = fma(-nm1[j], lim, Pn[j]); }  // uniform; adds exact zeros otherwise
            // l_x = -L q, q = limit - x on the violated side: the bits of -pen (max - x), -pen (min - x)
            lx = pen * fmax(xv - smax_v, 0.0) - pen * fmax(smin_v - xv, 0.0);
        }
        if (MR > 0) {
            UNR for (int rr = 0; rr < MRR; rr++) {
                if (PRP) {  // I_k and lam + I_k g of the preparing wave (which also updated and stored the multiplier)
                    Isk[rr] = pe1.y;
                    const double wI = Av[rr] * Isk[rr];
                    UNR for (int j = 0; j < N; j++) Pn[j] = fma(wI, Arow[rr][j], Pn[j]);
                    lx += Av[rr] * pe2.x;
                } else if (MR == 1 || rr < m) {
                    // g = A_r . x - b: every lane multiplies its own component, 8-lane butterfly (lane 7 adds 0); all lanes of the instance hold it
                    const double gr = oct_row_g(Av[rr], xv, bbr[rr]);
                    if (FUSED) {  // AL-ILQR.cpp:190 (mask with the multipliers before the update), :202-208 (update)
                        Isk[rr] = sw.pen_in * ((gr < 0 && lam[rr] == 0) ? 0.0 : 1.0);
                        const double nv = fma(sw.pen_update_prev, gr, lam[rr]);  // (k_apply's expression on this path)
                        const double nl = nv > 0 ? nv : 0;  // cwiseMax(0); a NaN becomes 0 as before
                        lam[rr] = upd ? nl : lam[rr];
                        if (upd && l == 0) stg(a.lambda, oLw + rofs[rr], lam[rr]);
                    }
                    const double wI = Av[rr] * Isk[rr];
                    UNR for (int j = 0; j < N; j++) Pn[j] = fma(wI, Arow[rr][j], Pn[j]);
                    lx += Av[rr] * (lam[rr] + Isk[rr] * gr);
                }
            }
        }
        // ---- P' = l_xx - (D N + reg N'N)/dt^2: row r of N'N = sum_k (N')_rk (row k of N), accumulated onto the rest
        fmac_rows_all<LPI>(Pn, Nn, ntc);
        UNR for (int j = 0; j < N; j++) P[j] = Pn[j];
        const double Md = UNIF ? nrc * row_dot_bc<LPI>(s, dv) : row_dot_bc<LPI>(M, dv);
        p = lx + p - (Qu + Dv * dv) * idt - reg * (Dv * Md - dv) * idt;
        if (FUSED && MR > 0) oLw -= Lstep;
      }
      if (IOW) k0 = gave_up ? 0 : k0;  // (a select on the loop counter, no branch: the loop ends here)
    }
    if (IOW && gave_up) {  // the I/O wave is gone: the wave's instances are out of the solve, whatever was stored for them
        if (l == 0 && b < d.B) { a.active[bb] = 0; atomicOr(&a.status[bb], ILQR_STATUS_SWEEP_IO); }
        return;
    }
    if (!IOK && (T - 2) % PF == PF - 1) {  // the last real step closed its group: no dummy step sent its image out
        UNR for (int q = 0; q < NPQ; q++) if (pst[q]) reinterpret_cast<double2*>(Kout + Kstep)[lane + 64 * q] = reinterpret_cast<const double2*>(sK[(PF - 1) & 1])[lane + 64 * q];
    }
    if (FUSED && acc && l == 0) {  // the acceptance is complete: the other buffer is the instance's trajectory now
        a.cur[bb] = 1 - cur;
        a.pend[bb] = 0;
    }
}

constexpr int SW_IO = 3;  // what the I/O wave carries: the gain records and the accepted x, u (the stages that were measured: profiles/sweep_io_variations.txt)
constexpr int SW_IO_PREP = SW_IO | 4;  // ... with the two preparing waves
constexpr int SW_DENSE = 8;            // the dense form (no I/O wave): every step's l_x | l_xx from SweepArgs::sd
template <int LPI, bool FUSED, bool UNIF, bool WG = false, int IO = 0>
static void launch_dpp2(bool al, const Bufs& a, int B, hipStream_t st, const SweepArgs& sw) {
    constexpr int IWG = (WG ? SW_WAVES : 1) * (64 / LPI);  // instances per workgroup
    const dim3 grid(grid_x8((B + IWG - 1) / IWG)), block(WG ? (SW_WAVES + ((IO & 7) ? 1 : 0) + ((IO & 4) ? SW_PREP : 0)) * 64 : 64);
    if (!al || a.m == 0) hipLaunchKernelGGL((k_backward_si_dpp<LPI, 0, FUSED, UNIF, WG, IO>), grid, block, 0, st, a, sw);
    else if (a.m <= 1) hipLaunchKernelGGL((k_backward_si_dpp<LPI, 1, FUSED, UNIF, WG, IO>), grid, block, 0, st, a, sw);
    else if constexpr ((IO & 7) == 0) hipLaunchKernelGGL((k_backward_si_dpp<LPI, 4, FUSED, UNIF, WG, IO>), grid, block, 0, st, a, sw);
}

// The dense instantiations live in a translation unit of their own (ilqr_kernels_dpp_dense.hip, which includes this file with
// ILQR_DPP_DENSE_TU defined): with them in this unit's code object every existing kernel moved by 0x4900 bytes, and the C3 bench line follows
// the placement of its kernels (ilqr_multistart_kernels.hpp).  This unit's kernels are the parent's, where the parent had them.
void launch_dpp_dense(bool al, bool uniform_R, int lpi, const Bufs& a, int B, hipStream_t st, const SweepArgs& sw);
#ifndef ILQR_DPP_DENSE_TU
void launch_backward_si_dpp(bool al, bool fused, bool uniform_R, int lpi, const Bufs& a, int B, hipStream_t st, const SweepArgs& sw) {
    if (sw.sd && !fused) return launch_dpp_dense(al, uniform_R, lpi, a, B, st, sw);
    if (lpi == 16 && fused && sw.si_wg && sw.si_io && sw.si_prep && (!al || a.m <= 1)) {  // ... with the I/O wave and the preparing waves (RiccatiPlan::si_prep)
        if (uniform_R) launch_dpp2<16, true, true, true, SW_IO_PREP>(al, a, B, st, sw); else launch_dpp2<16, true, false, true, SW_IO_PREP>(al, a, B, st, sw);
    } else if (lpi == 16 && fused && sw.si_wg && sw.si_io && (!al || a.m <= 1)) {  // ... with the I/O wave (RiccatiPlan::si_io): at most one constraint row
        if (uniform_R) launch_dpp2<16, true, true, true, SW_IO>(al, a, B, st, sw); else launch_dpp2<16, true, false, true, SW_IO>(al, a, B, st, sw);
    } else if (lpi == 16 && fused && sw.si_wg) {  // the workgroup form (RiccatiPlan::si_wg): instantiated for the fused acceptance only
        if (uniform_R) launch_dpp2<16, true, true, true>(al, a, B, st, sw); else launch_dpp2<16, true, false, true>(al, a, B, st, sw);
    } else if (lpi == 16) {
        if (fused) { if (uniform_R) launch_dpp2<16, true, true>(al, a, B, st, sw); else launch_dpp2<16, true, false>(al, a, B, st, sw); }
        else { if (uniform_R) launch_dpp2<16, false, true>(al, a, B, st, sw); else launch_dpp2<16, false, false>(al, a, B, st, sw); }
    } else {
        if (fused) { if (uniform_R) launch_dpp2<8, true, true>(al, a, B, st, sw); else launch_dpp2<8, true, false>(al, a, B, st, sw); }
        else { if (uniform_R) launch_dpp2<8, false, true>(al, a, B, st, sw); else launch_dpp2<8, false, false>(al, a, B, st, sw); }
    }
}

#else
// the dense form (RiccatiPlan::obs_dense): lone waves, either grouping
void launch_dpp_dense(bool al, bool uniform_R, int lpi, const Bufs& a, int B, hipStream_t st, const SweepArgs& sw) {
    if (lpi == 16) { if (uniform_R) launch_dpp2<16, false, true, false, SW_DENSE>(al, a, B, st, sw); else launch_dpp2<16, false, false, false, SW_DENSE>(al, a, B, st, sw); }
    else { if (uniform_R) launch_dpp2<8, false, true, false, SW_DENSE>(al, a, B, st, sw); else launch_dpp2<8, false, false, false, SW_DENSE>(al, a, B, st, sw); }
}
#endif

}  // namespace ilqr
