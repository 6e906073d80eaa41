// ilqr_capi_internal.hpp -- what the units of the C ABI (ilqr_capi_*.cpp) share: the problem behind the opaque ilqr_problem, the grow-only device
// buffer, the staging cursor of the host-pointer calls, the profiling marks and the few functions that cross units.  Internal: not installed.
//
// Host-side orchestration only: lowering of the POD problem description to the device descriptor, buffer ownership, layout conversion at the
// boundary and the launch sequences.  No CPU fallback exists: every entry point fails loudly if HIP does.
#pragma once
#include "../../include/ilqr_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "ilqr_batchcp.hpp"
#include "ilqr_clearance.hpp"
#include "ilqr_closed_loop.hpp"
#include "ilqr_closed_loop_cov.hpp"
#include "ilqr_cov_clearance.hpp"
#include "ilqr_ctx.hpp"
#include "ilqr_kernels.hpp"
#include "ilqr_multistart.hpp"
#include "ilqr_obstacle.hpp"
#include "ilqr_plan.hpp"

using namespace ilqr;  // this header is for the units of the C ABI alone

namespace ilqr_capi {

// A device buffer of bytes that only grows: the staging areas of the host-pointer calls and the workspaces of the closed loop and of clearance.
// A call whose need is covered allocates nothing; growing waits for the stream first, since kernels in flight may still read the old buffer.
struct DevScratch {
    void* ptr = nullptr;
    size_t bytes = 0;
    int reserve(ilqr_ctx* c, size_t n) {
        if (bytes >= n) return 0;
        if (ptr) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(ptr)); ptr = nullptr; bytes = 0; }
        HIPCHK(c, hipMalloc(&ptr, n));
        bytes = n;
        return 0;
    }
    int reserve_doubles(ilqr_ctx* c, size_t n) { return reserve(c, n * sizeof(double)); }
    double* doubles() const { return (double*)ptr; }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
};

// The staging area of a host-pointer call, laid out by one cursor: every slice is the next n elements (doubles or ints; ilqr_fk_batch also stages
// its descriptor), 8-byte aligned.  lay() walks the caller's list of slices twice, first without a base, which gives the size to reserve (nothing
// is copied or noted), then over the reserved area: the size cannot disagree with the walk.  So the list must read the caller's pointers and write
// only the device-side ones.  fetch() copies every take_out slice to its host array and waits for the stream.
struct Staging {
    ilqr_ctx* c;
    char* base = nullptr;
    size_t used = 0;
    bool failed = false;  // a copy in has failed: the context holds the error
    struct Back { void* host; const void* dev; size_t bytes; };
    std::vector<Back> back;
    int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) { HIPCHK(c, hipMemcpyAsync(dst, src, bytes, kind, c->stream)); return 0; }
    template <class T>
    T* take(size_t n) {
        static_assert(std::is_trivially_copyable<T>::value && alignof(T) <= 8, "slices are raw bytes at 8-byte boundaries");
        const size_t at = used;
        used += (n * sizeof(T) + 7) / 8 * 8;
        return base ? (T*)(base + at) : nullptr;
    }
    template <class T>
    const T* take_in(const T* host, size_t n) {  // ... filled with the caller's input
        T* s = take<T>(n);
        if (base && n && copy(s, host, n * sizeof(T), hipMemcpyHostToDevice)) failed = true;
        return s;
    }
    template <class T>
    T* take_out(T* host, size_t n) {  // ... which fetch copies to `host`, where there is one
        T* s = take<T>(n);
        if (base && host && n) back.push_back({host, s, n * sizeof(T)});
        return s;
    }
    // size, reserve, walk again: slices(Staging&) names every slice of the call, and may return non-zero to refuse
    template <class F>
    int lay(DevScratch& buf, F&& slices) {
        for (int walk = 0; walk < 2; walk++) {
            used = 0;
            if constexpr (std::is_void<decltype(slices(*this))>::value) slices(*this);
            else if (slices(*this)) return 1;
            if (walk == 0) {
                if (buf.reserve(c, used)) return 1;
                base = (char*)buf.ptr;
            }
        }
        return failed ? 1 : 0;
    }
    int fetch() {
        for (const Back& b : back)
            if (copy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost)) return 1;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    }
};
}  // namespace ilqr_capi

struct ilqr_problem {
    ilqr_ctx* ctx = nullptr;
    ilqr_problem_desc desc;  // as given: the user's dof
    ilqr_dims udims;         // the user's dimensions: every array crossing the ABI
    ilqr_dims dims;          // the device's (7 joints): every device buffer
    DofMap map;              // user index -> device index (ilqr_dofmap.hpp)
    bool mapped = false;     // dof < 7: the layout conversions go through `map`; a 7-joint problem takes the plain ones
    IndexMap qmap;           // q0 / dq0: [dof] -> [7]
    int B = 0, Bp = 0, T = 0;
    DevDesc hdesc;
    DevDesc* ddesc = nullptr;
    DevDesc* ddesc_half[2] = {nullptr, nullptr};  // the descriptor with B = the half's instance count (split solves)
    int half_b0[2] = {0, 0}, half_B[2] = {0, 0};
    Bufs bufs;
    std::vector<void*> allocs;
    double *conA = nullptr, *conb = nullptr;  // device copies of the shared constraint rows
    double* lambda0 = nullptr;                // initial multipliers, kept for ilqr_problem_reset_multipliers
    bool con_state_only = false;              // no constraint row touches the controls (enables the closed-form sweep)
    int trace_iters = 0;
    ilqr_capi::DevScratch staging;  // device staging of every host-pointer call (Staging)
    int last_nb_iter = 0;
    bool has_controls = false, has_state = false;
    bool has_gains = false;  // a Riccati solve with nb_iter >= 1 or ilqr_problem_gains has run since the inputs last changed: X, U, KD are one plan (closed_loop)
    bool has_plan = false;   // one of the four solvers has run since the inputs last changed: X, U are a plan ilqr_problem_gains can sweep about
    ilqr_capi::DevScratch cl_cost;  // closed_loop_noise without a cost array: the per-sample costs k_closed_loop_stats reduces
    ilqr_capi::DevScratch cl_kpx;   // closed_loop: state | control of every sample at the step-table entries (k_closed_loop_coop -> k_closed_loop_kp)
    ilqr_capi::DevScratch cl_rep;   // closed_loop_report through device pointers: kp_err | lim_cost where the caller asks only for their reductions
    ilqr_capi::DevScratch cl_con_ws;   // closed_loop_report_con through device pointers: con_max | con_steps where the caller asks only for their reductions
    ilqr_capi::DevScratch cl_cov_ws;   // closed_loop_cov: the per-lane matrices of the generic kernel k_cl_cov
    ilqr_capi::DevScratch cl_cov_kps;  // closed_loop_cov through device pointers: kp_Sigma where the caller asks only for kp_var
    // obstacle terms of the stage cost (ilqr_problem_set_obstacles): the geometry, the obstacle sets and the slots of k_obs_derivs are device
    // memory of this problem; `obs` is what the kernels are given.  Problems with these terms run on the generic kernels unless the context's
    // obstacle path sends them to the cooperative ones (plan_input).
    bool has_obs = false;
    ObsProblem obs = {};
    size_t obs_sets_bytes = 0;
    // the cooperative path of these terms (RiccatiPlan::obs_dense), allocated at its first solve: l_x | l_xx of every stage (one kpd entry per
    // step) and the obstacle cost of every (step, step size) of a line search
    ObsDense obs_dense = {};
    bool u0_zero = false;  // the initial controls given from the host are all zero (lets the wide-basis batch solver skip their projection)
    BatchCPState cp;
    BatchWideState cpw;
};

namespace ilqr_capi {

template <class T>
int dalloc(ilqr_problem* p, T** ptr, size_t n, bool zero = true) {
    void* q = nullptr;
    if (n == 0) n = 1;
    HIPCHK(p->ctx, hipMalloc(&q, n * sizeof(T)));
    p->allocs.push_back(q);
    if (zero) HIPCHK(p->ctx, hipMemsetAsync(q, 0, n * sizeof(T), p->ctx->stream));
    *ptr = (T*)q;
    return 0;
}

// profiling (ilqr_capi_ctx.cpp): one event in front of every kernel launch; which < 0 is the end mark of a call
void prof_mark(ilqr_ctx* c, int which);
struct ProfScope {  // marks the launch that follows; the interval is closed by the next mark
    ProfScope(ilqr_ctx* c, int w) { prof_mark(c, w); }
};
ProfHook prof_hook(ilqr_ctx* c);

int lower_chain(ilqr_ctx* c, const ilqr_problem_desc& d, DevChain& ch);  // ilqr_capi_problem.cpp
void clr_release(ilqr_ctx* c);  // the clearance calls' buffers (ilqr_capi_clearance.cpp)
// What ilqr_problem_closed_loop_cov_clr shares with the clearance calls (ilqr_capi_clearance.cpp).  clr_check_world: their refusals about robot,
// planes, obstacles, sets and the chain, under the name fn.  clr_bind_geom: the context's geometry block holds this call's geometry (uploaded
// where it differs from the previous call's); n_anchor is the geometry's.  clr_cov_scratch: the context's buffers of that call -- 0: Sigma where
// the caller does not ask for it, 1: the keys of k_cov_clr.
int clr_check_world(ilqr_ctx* c, const std::string& fn, const ilqr_problem_desc& d, int n, int T, const ilqr_clr_robot* rb, const ilqr_clr_world* w, bool dev);
int clr_bind_geom(ilqr_ctx* c, const ilqr_problem_desc& d, const ilqr_clr_robot& rb, const ClrGeom** geom, int* n_anchor);
DevScratch& clr_cov_scratch(ilqr_ctx* c, int which);

// A geometry with self pairs (ObsProblem::n_anchor > 0) takes the ObsSelfArgs forms of the three kernels that read the obstacle terms
// (ilqr_obstacle.hpp); o is null for a problem without the terms.
inline void launch_init_obs(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st, double penalty, const ObsProblem* o) {
    if (o && o->n_anchor) launch_init_self(kind, nd, al, a, B, st, penalty, *o);
    else launch_init(kind, nd, al, a, B, st, penalty, o);
}
inline void launch_forward_generic_obs(int kind, int nd, bool al, const Bufs& a, int B, hipStream_t st, const FwdArgs& f, const ObsProblem* o) {
    if (o && o->n_anchor) launch_forward_generic_self(kind, nd, al, a, B, st, f, *o);
    else launch_forward_generic(kind, nd, al, a, B, st, f, o);
}
inline void launch_obs_derivs_any(const Bufs& a, const ObsProblem& o, int B, int T, int nx, int all, hipStream_t st) {
    if (o.n_anchor) launch_obs_derivs_self(a, o, B, T, nx, all, st);
    else launch_obs_derivs(a, o, B, T, nx, all, st);
}

}  // namespace ilqr_capi
