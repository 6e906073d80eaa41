// Everything of the library that is NOT the lane-per-instance kernel set: refused on the host harness (see hip/hip_runtime.h).
#include <hip/hip_runtime.h>

#include <string>

#include "ilqr_batchcp.hpp"
#include "ilqr_kernels.hpp"

thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace ilqr {
[[noreturn]] static void refuse(const char* what) {
    std::fprintf(stderr, "hostsim: %s is a cooperative GPU kernel and cannot run on the sanitizer harness (use ILQR_HIP_PATH=v1)\n", what);
    std::abort();
}
void launch_al_update(int, int, const Bufs&, int, int, hipStream_t, const FwdArgs&) { refuse("k_al_post"); }
void launch_backward_si_dpp(bool, bool, bool, int, const Bufs&, int, hipStream_t, const SweepArgs&) { refuse("k_backward_si_dpp"); }
void launch_backward_mfma(int, int, bool, const Bufs&, int, hipStream_t) { refuse("k_backward_mfma"); }
void launch_backward_rows(int, int, bool, const Bufs&, int, hipStream_t) { refuse("k_backward_rows"); }
void launch_apply_tm(int, int, bool, const Bufs&, int, hipStream_t, const FwdArgs&) { refuse("k_apply_rows_tm"); }
void launch_forward_tm(int, int, const Bufs&, int, hipStream_t, const FwdArgs&) { refuse("k_forward_mfma"); }
void launch_forward_lin(const Bufs&, int, hipStream_t, const FwdArgs&) { refuse("k_forward_lin"); }
void launch_apply_lin(const Bufs&, int, int, hipStream_t) { refuse("k_blend"); }
void launch_init_lti(int, int, const Bufs&, int, hipStream_t) { refuse("k_init_roll_lti"); }
void launch_forward_wave(int, bool, const Bufs&, int, hipStream_t, const FwdArgs&) { refuse("k_forward_wg"); }
void launch_apply_wave(int, const Bufs&, int, int, hipStream_t, const FwdArgs&) { refuse("k_apply"); }
int batchwide_solve(BatchWideState&, const DevDesc&, Bufs&, int, int, const double*, int, int, int, bool, hipStream_t, std::string&, const ProfHook&) { refuse("batchwide_solve"); }
void batchwide_free(BatchWideState&) {}
int batchcp_solve(BatchCPState&, const DevDesc&, Bufs&, int, int, int, int, const double*, int, int, int, hipStream_t, std::string&, const ProfHook&) { refuse("batchcp_solve"); }
void batchcp_free(BatchCPState&) {}
}  // namespace ilqr
