// ilqr_lanes.hpp -- lane-level building blocks of the cooperative kernels (gfx950, fp64, device code only): moves of a double between the
// lanes of a wave, the sums built on them, the ring move, the LDS ordering helpers and the flag words (with their bounded poll) by which the waves of a workgroup hand work to each other.  One definition each; the inline-assembly DPP
// blocks (v_fmac_f64_dpp strings and their bank masks) stay in the kernel files that schedule them by hand.
// Not for ilqr_kernels.hip, ilqr_step.hpp or ilqr_device.hpp: tests/tools/hostsim compiles those with g++.
#pragma once
#include <hip/hip_runtime.h>

namespace ilqr {

// compiler barrier between LDS accesses of one wave (they execute in order: nothing to wait for, only to keep in place)
#define LDS_ORDER() asm volatile("" ::: "memory")
// Workgroup barrier that only drains LDS traffic (__syncthreads() also emits s_waitcnt vmcnt(0): it would wait for loads
// prefetched steps ahead).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ------------------------------------------------------------------------------------------------ flag words in LDS (k_backward_si_dpp, k_forward_reg)
// LDS byte address of a __shared__ object (for inline assembly)
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)(const __attribute__((address_space(3))) void*)p; }
// Flag words in LDS: plain ds_read / ds_write kept in place by compiler barriers.  (Not `volatile`: through a generic pointer that is a flat
// access, which counts in vmcnt too and made every step of the chain wait for its prefetched loads -- vmcnt(0).)
typedef __attribute__((address_space(3))) int lds_int;
__device__ __forceinline__ int flag_read(const int* p) { LDS_ORDER(); const int v = *(const lds_int*)p; LDS_ORDER(); return v; }
__device__ __forceinline__ void flag_write(int* p, int v) { LDS_ORDER(); *(lds_int*)p = v; LDS_ORDER(); }
// Bounded wait of a wave for a flag word (LDS byte address `addr`, last read as `seen`) to reach `need`: polls at most `polls` times with
// s_sleep 1 between the polls and returns 1 if it gave up.  One asm statement: no control flow for the compiler.
__device__ __forceinline__ int flag_wait_ge(int seen, unsigned addr, int need, int polls) {
    int v = seen, cons, cnt;
    asm volatile(
        "s_mov_b32 %[cnt], 0\n"
        "1:\n\t"
        "v_readfirstlane_b32 %[cons], %[v]\n\t"
        "s_cmp_ge_i32 %[cons], %[need]\n\t"
        "s_cbranch_scc1 2f\n\t"
        "s_cmp_ge_u32 %[cnt], %[lim]\n\t"
        "s_cbranch_scc1 2f\n\t"
        "s_sleep 1\n\t"
        "ds_read_b32 %[v], %[addr]\n\t"
        "s_add_u32 %[cnt], %[cnt], 1\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "s_branch 1b\n"
        "2:"
        : [v] "+v"(v), [cons] "=&s"(cons), [cnt] "=&s"(cnt)
        : [addr] "v"(addr), [need] "s"(need), [lim] "s"(polls)
        : "memory", "scc");
    return __builtin_amdgcn_readfirstlane(cons < need ? 1 : 0);  // (uniform by construction; the compiler takes asm results for divergent)
}

// ------------------------------------------------------------------------------------------------ moves
// DPP move of a double by its 32-bit halves, CTRL = the DPP control word.  For patterns in which every lane has a source: no "old"
// operand, no copy.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// The same move on the whole double with 0 for the lanes that have no source (shifts), in the compiler-visible form: the compiler
// handles the hazards and may fold the move into its user.
template <int CTRL>
__device__ __forceinline__ double dppz_f64(double v) {
    return __builtin_amdgcn_update_dpp(0.0, v, CTRL, 0xf, 0xf, false);
}
template <int L>
__device__ __forceinline__ double dppz_bcast(double v) { return dppz_f64<0x150 + L>(v); }  // lane L of the DPP row to all sixteen
// lane LO of the DPP row to its lanes 0 .. 7, lane HI to its lanes 8 .. 15 (bank masks: a bank is four lanes); HI < 0: `other` there instead
template <int LO, int HI>
__device__ __forceinline__ double dpp_bcast_halves(double v, double other = 0.0) {
    const double hi = HI < 0 ? other : __builtin_amdgcn_update_dpp(0.0, v, 0x150 + (HI < 0 ? 0 : HI), 0xf, 0xc, false);
    return __builtin_amdgcn_update_dpp(hi, v, 0x150 + LO, 0xf, 0x3, false);
}
__device__ __forceinline__ double dppz_shr7(double v) { return dppz_f64<0x117>(v); }  // lane l <- lane l - 7 (0 below)
__device__ __forceinline__ double dppz_shl7(double v) { return dppz_f64<0x107>(v); }  // lane l <- lane l + 7 (0 above)
// v of the lane at byte address 4 * lane (ds_bpermute: LDS crossbar, no LDS memory)
__device__ __forceinline__ double bperm_f64(int byte_addr, double v) {
    const int lo = __builtin_amdgcn_ds_bpermute(byte_addr, __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute(byte_addr, __double2hiint(v));
    return __hiloint2double(hi, lo);
}
// A ring value moved out of its slot by an instruction the compiler cannot fold away: the slot register is then free BEFORE the slot's next
// load is issued, the loop-carried value and the load destination share one register, and no copy is left on the back edge.  (Without it
// the old value stayed in place for the whole step, the new load went to a second register, and the copies that rotate the ring at the
// end of the unrolled group waited for the loads issued ONE step earlier: s_waitcnt vmcnt(4) .. vmcnt(0) once per group.)
__device__ __forceinline__ double ring_take(double v) {
    double r;
    asm volatile("v_mov_b64_e32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}

// ------------------------------------------------------------------------------------------------ sums, result in every lane of the group
// the 4 lanes of a quad (quad_perm [1,0,3,2] then [2,3,0,1])
__device__ __forceinline__ double quad_sum(double v) {
    v += dpp_f64<0xB1>(v);
    v += dpp_f64<0x4E>(v);
    return v;
}
// lanes 8m .. 8m+7 (then row_half_mirror)
__device__ __forceinline__ double oct_sum(double v) {
    v = quad_sum(v);
    v += dpp_f64<0x141>(v);
    return v;
}
// The same sum with every addition rounded on its own: left to contraction, the first one became fma(a_l, x_l, a_l' x_l') in each lane --
// another value in lane l than in its partner l', so the lanes of an instance disagreed in the last bits of g (and could disagree on the
// sign of a g at zero), and no other kernel could restate the sum.  As written it is the tree
// ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)) in every lane: con_g_oct (ilqr_kernels_wave.hip) gives the same bits.
__device__ __forceinline__ double oct_sum_rounded(double v) {
#pragma clang fp contract(off)
    v = v + dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
    v = v + dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
    v = v + dpp_f64<0x141>(v);  // row_half_mirror
    return v;
}
// the 16 lanes of a DPP row (then row_mirror)
__device__ __forceinline__ double row16_sum(double v) {
    v = oct_sum(v);
    v += dpp_f64<0x140>(v);
    return v;
}
// lanes c, c+16, c+32, c+48: the same lane of the four rows
__device__ __forceinline__ double cross_rows_sum(double v) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) { return cross_rows_sum(row16_sum(v)); }

}  // namespace ilqr
