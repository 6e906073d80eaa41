// ilqr_pivots.hpp -- Gauss-Jordan inversion of a small SPD matrix in registers (device code; included by .hip files only).
// Shared by the backward sweep of ilqr_kernels_mfma.hip and the LQT Riccati chain of ilqr_lqt.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace ilqr {

// ---- Quu + reg I inverted in REGISTERS (round 3).  The 8 x 8 matrix was swept in LDS, one entry per lane: per pivot three dependent LDS
// reads, the reciprocal, one FMA and an LDS write -- ~280 clocks of a lone wave's chain, eight times per step, more than half of the
// step.  Now every lane reads ROW (c16 & 7) of the matrix once (the four DPP rows of the wave hold four copies) and the pivots run as in
// ilqr_kernels_dpp.hip: the pivot row is the DPP operand of the FMA (v_fmac_f64_dpp ... row_newbcast:c), deferred row scaling, no LDS.
// NP pivots (= n_u: 7 or 8; the LQT chain pads S to 8 with an identity tail) over NP columns; afterwards -myrc * s is this lane's row of the inverse.
// Hazards as explained there (two wait states before a DPP read of a freshly written register).
#define MPV_ALL_ " row_mask:0xf bank_mask:0xf"
#define MPV_HEAD_(C) "v_mov_b64_dpp %[acc], %[s" #C "] row_newbcast:" #C MPV_ALL_ "\n\t"
#define MPV_RCP_(C)                                                                        \
    "v_rcp_f64 %[rc], %[acc]\n\t"                                                          \
    "v_fma_f64 %[t], %[s" #C "], %[n" #C "], %[s" #C "]\n\t"                               \
    "v_fma_f64 %[e], -%[acc], %[rc], 1.0\n\t"                                              \
    "v_fma_f64 %[e], %[e], %[e], %[e]\n\t"                                                 \
    "v_fma_f64 %[rc], %[e], %[rc], %[rc]\n\t"                                              \
    "v_mul_f64 %[t], %[t], %[rc]\n\t"
#define MPV_F_(J, C) "v_fmac_f64_dpp %[s" #J "], %[s" #J "], -%[t] row_newbcast:" #C MPV_ALL_ "\n\t"
#define MPV_TAIL_(C) "v_add_f64 %[s" #C "], %[t], %[n" #C "]\n\tv_fma_f64 %[myrc], -%[rc], %[n" #C "], %[myrc]\n\t"
#define MPV7_(C, A, B, D, E, F, G) MPV_HEAD_(C) MPV_RCP_(C) MPV_F_(A, C) MPV_F_(B, C) MPV_F_(D, C) MPV_F_(E, C) MPV_F_(F, C) MPV_F_(G, C) MPV_TAIL_(C)
#define MPV8_(C, A, B, D, E, F, G, H) MPV_HEAD_(C) MPV_RCP_(C) MPV_F_(A, C) MPV_F_(B, C) MPV_F_(D, C) MPV_F_(E, C) MPV_F_(F, C) MPV_F_(G, C) MPV_F_(H, C) MPV_TAIL_(C)
template <int NP>
__device__ __forceinline__ void quu_pivots(double (&s)[8], const double (&nm1)[8], double& myrc) {
    double acc, rc, e, t;
    if (NP == 8) {
        asm volatile("s_nop 1\n\t" MPV8_(0, 1, 2, 3, 4, 5, 6, 7) MPV8_(1, 0, 2, 3, 4, 5, 6, 7) MPV8_(2, 0, 1, 3, 4, 5, 6, 7) MPV8_(3, 0, 1, 2, 4, 5, 6, 7)
                         MPV8_(4, 0, 1, 2, 3, 5, 6, 7) MPV8_(5, 0, 1, 2, 3, 4, 6, 7) MPV8_(6, 0, 1, 2, 3, 4, 5, 7) MPV8_(7, 0, 1, 2, 3, 4, 5, 6) "s_nop 0"
                     : [acc] "=&v"(acc), [rc] "=&v"(rc), [e] "=&v"(e), [t] "=&v"(t), [s0] "+v"(s[0]), [s1] "+v"(s[1]), [s2] "+v"(s[2]), [s3] "+v"(s[3]),
                       [s4] "+v"(s[4]), [s5] "+v"(s[5]), [s6] "+v"(s[6]), [s7] "+v"(s[7]), [myrc] "+v"(myrc)
                     : [n0] "v"(nm1[0]), [n1] "v"(nm1[1]), [n2] "v"(nm1[2]), [n3] "v"(nm1[3]), [n4] "v"(nm1[4]), [n5] "v"(nm1[5]), [n6] "v"(nm1[6]), [n7] "v"(nm1[7]));
    } else {
        asm volatile("s_nop 1\n\t" MPV7_(0, 1, 2, 3, 4, 5, 6) MPV7_(1, 0, 2, 3, 4, 5, 6) MPV7_(2, 0, 1, 3, 4, 5, 6) MPV7_(3, 0, 1, 2, 4, 5, 6) MPV7_(4, 0, 1, 2, 3, 5, 6)
                         MPV7_(5, 0, 1, 2, 3, 4, 6) MPV7_(6, 0, 1, 2, 3, 4, 5) "s_nop 0"
                     : [acc] "=&v"(acc), [rc] "=&v"(rc), [e] "=&v"(e), [t] "=&v"(t), [s0] "+v"(s[0]), [s1] "+v"(s[1]), [s2] "+v"(s[2]), [s3] "+v"(s[3]),
                       [s4] "+v"(s[4]), [s5] "+v"(s[5]), [s6] "+v"(s[6]), [myrc] "+v"(myrc)
                     : [n0] "v"(nm1[0]), [n1] "v"(nm1[1]), [n2] "v"(nm1[2]), [n3] "v"(nm1[3]), [n4] "v"(nm1[4]), [n5] "v"(nm1[5]), [n6] "v"(nm1[6]));
    }
}

}  // namespace ilqr
