// ilqr_ctx.hpp -- the context behind the opaque ilqr_ctx of include/ilqr_hip.h, shared by the translation units of the C ABI
// (ilqr_capi_*.cpp, ilqr_lqt.cpp).  Internal: not installed, not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/ilqr_hip.h"
#include "ilqr_plan.hpp"

struct ilqr_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    bool profile = false;
    int split = 1;  // ilqr_ctx_set_split: 0 off, 1 where it was measured to pay, 2 every cooperative path (experiments)
    double prof_ms[ILQR_PROF_COUNT] = {0, 0, 0, 0, 0};
    int prof_n[ILQR_PROF_COUNT] = {0, 0, 0, 0, 0};
    struct Pending { hipEvent_t a, b; int which; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    std::vector<ilqr_problem*> problems;  // live problems of this context (destroyed with it)
    // other handles of this context (LQT batches, ilqr_lqt.cpp), destroyed with it: the destroy function and its handle.  A list of
    // callbacks keeps this file free of references to their translation units.
    struct Cleanup { void (*destroy)(void*); void* handle; };
    std::vector<Cleanup> cleanups;
    struct ClrState* clr = nullptr;  // the clearance calls' geometry buffer and workspace (ilqr_capi_clearance.cpp), made by the first call and reused
    // split solves (solve_riccati): the two halves of a batch run on their own streams, joined to `stream` by events
    int n_simd = 1024;  // SIMDs of the device (4 per CU)
    bool xc_generic = false, xc_cp_lane = false, xc_cp_general = false;  // cross-check kernel variants (ilqr_ctx_set_crosscheck)
    bool obs_coop = false;  // ilqr_ctx_set_obstacle_path: problems with obstacle terms may take the cooperative kernels (state of its own: no pin touches it)
    ilqr::SweepPin xc_sweep = ilqr::SweepPin::Auto;      // variant pins (ILQR_XC_*): sweep of the 2nd-order / time systems,
    ilqr::FwdPin xc_forward = ilqr::FwdPin::Auto;        // forward pass of the single-integrator systems,
    ilqr::RerollPin xc_reroll = ilqr::RerollPin::Auto;   // re-roll of the line-search winner on the time systems
    hipStream_t half_stream[2] = {nullptr, nullptr};
    hipEvent_t ev_begin = nullptr, ev_half_done[2] = {nullptr, nullptr}, ev_stagger = nullptr;
};

static inline int fail(ilqr_ctx* c, const std::string& m) {
    if (c) c->err = m;
    return 1;
}
#define HIPCHK(ctx, call)                                                                                  \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess) return fail((ctx), std::string(#call) + ": " + hipGetErrorString(e_));       \
    } while (0)

