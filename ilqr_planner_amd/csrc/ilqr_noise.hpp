// ilqr_noise.hpp -- the counter-based generator of the closed-loop rollouts' disturbances (ilqr_problem_closed_loop_noise).  Plain C++: the
// kernels (hipcc), the host build of the generic kernel set (g++) and tests/cpp/philox_main.cpp compile the same text.  The definition is part
// of the public contract and is restated in include/ilqr_hip.h.
//
//   Philox4x32-10 (Salmon et al., SC'11): counter (c0, c1, c2, c3), key (k0, k1); ten rounds of
//       p0 = M0 c0, p1 = M1 c2;  c <- (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0));  k0 += W0, k1 += W1
//   key = (seed & 0xffffffff, seed >> 32); counter = (global instance, global sample, step, pair); step 0xFFFFFFFF is the start-state draw.
//   One call gives two normals (Box-Muller on two 53-bit uniforms of (0, 1]):
//       u1 = ((r1:r0 >> 11) + 0.5) 2^-53, u2 likewise from r3:r2;  z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2 ln u1) sin(2 pi u2)
//   Pair j serves entries 2j and 2j + 1 of the user's state layout.
// The draw of a (instance, sample, step) depends on nothing else, so a cut-out of a batch, a shard or a range of samples reproduces the
// large call; it does not depend on the state chain either, so a kernel may issue it ahead of the step that uses it.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef ILQR_DEV
#define ILQR_DEV inline
#endif

namespace ilqr {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
constexpr uint32_t NOISE_STEP_START = 0xFFFFFFFFu;   // the step index of the start-state draw

ILQR_DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// a uniform of (0, 1] from the 53 high bits of hi:lo (from 2^52 on the + 0.5 is rounded away; the top value gives 1.0: ln 1 = 0, a zero radius)
ILQR_DEV double noise_uniform(uint32_t lo, uint32_t hi) {
    return ((double)((((uint64_t)hi << 32) | lo) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

// the two normals of the Philox output r
ILQR_DEV void noise_normals(const uint32_t* r, double& z0, double& z1) {
    const double u1 = noise_uniform(r[0], r[1]), u2 = noise_uniform(r[2], r[3]);
    const double rad = sqrt(-2.0 * log(u1));
    double s, c;
#if defined(__HIP_DEVICE_COMPILE__)
    sincospi(2.0 * u2, &s, &c);   // no large-argument reduction path
#else
    const double a = M_PI * 2.0 * u2;
    s = sin(a);
    c = cos(a);
#endif
    z0 = rad * c;
    z1 = rad * s;
}

// pair j of step k of global (instance, sample)
ILQR_DEV void noise_pair(unsigned long long seed, uint32_t instance, uint32_t sample, uint32_t k, uint32_t j, double& z0, double& z1) {
    uint32_t r[4];
    philox4x32_10(instance, sample, k, j, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), r);
    noise_normals(r, z0, z1);
}

// Pair j of the draw below: its two normals go to the device entries whose user entries are 2j and 2j + 1.
template <int NX, bool MAP>
ILQR_DEV void noise_draw_pair(unsigned long long seed, uint32_t instance, uint32_t sample, uint32_t k, int j, const double* sigma, int nxu, const int* usr,
                              double* nz, unsigned& on) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int i0 = 2 * j, i1 = 2 * j + 1;
    const double s0 = i0 < nxu ? sigma[i0] : 0.0;
    const double s1 = (i1 < NX && i1 < nxu) ? sigma[i1 < NX ? i1 : 0] : 0.0;
    if (s0 != 0.0 || s1 != 0.0) {
        double z0, z1;
        noise_pair(seed, instance, sample, k, (uint32_t)j, z0, z1);
        const double v0 = s0 * z0, v1 = s1 * z1;
#if defined(__clang__)
#pragma unroll
#endif
        for (int i = 0; i < NX; i++) {
            const int iu = MAP ? usr[i] : i;
            if (iu == i0 && s0 != 0.0) { nz[i] = v0; on |= 1u << i; }
            else if (iu == i1 && s1 != 0.0) { nz[i] = v1; on |= 1u << i; }
        }
    }
}

// The draw of one step for a state of NX device entries: nz[i] = sigma[user entry of i] * z (the product rounded on its own, so that a caller who
// adds the stored value reproduces the step) and bit i of the result set, for every device entry whose user entry has sigma != 0.  usr: the
// user entry of every device entry (a chain of fewer than 7 joints; padding < 0 gets nothing) where MAP, else the identity.  sigma and usr are
// wave-uniform: a pair whose sigmas are both 0 is not generated.  ROLL: one pair at a time in a rolled loop (every index into nz stays a
// constant: the entry is chosen by scalar compares) -- the same values with one pair's registers live at a time, for the generic kernel, which holds FK
// (unrolled, its 2nd-order instantiations reached 512 VGPRs and 28 to 228 B of scratch; rolled, 488 to 500 and none).
template <int NX, bool MAP, bool ROLL>
ILQR_DEV unsigned noise_draw(unsigned long long seed, uint32_t instance, uint32_t sample, uint32_t k, const double* sigma, int nxu, const int* usr,
                             double* nz) {
    unsigned on = 0;
    if (ROLL) {
#if defined(__clang__)
#pragma unroll 1
#endif
        for (int j = 0; j < (NX + 1) / 2; j++) noise_draw_pair<NX, MAP>(seed, instance, sample, k, j, sigma, nxu, usr, nz, on);
    } else {
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = 0; j < (NX + 1) / 2; j++) noise_draw_pair<NX, MAP>(seed, instance, sample, k, j, sigma, nxu, usr, nz, on);
    }
    return on;
}

}  // namespace ilqr
