// The LQT entry points of the C ABI (ilqr_lqt_capi.cpp, matrix-core kernels) for programs that link the host classes
// (csrc/host/ilqr_host.cpp) against the host build: refused, as the cooperative kernels are in stubs.cpp.
#include <cstdio>
#include <cstdlib>

#include "../../../include/ilqr_hip.h"

[[noreturn]] static void refuse(const char* what) {
    std::fprintf(stderr, "hostsim: %s needs the GPU library\n", what);
    std::abort();
}
extern "C" {
int ilqr_lqt_create(ilqr_ctx*, int, int, int, int, const double*, const double*, double, const double*, int, ilqr_lqt**) { refuse("ilqr_lqt_create"); }
void ilqr_lqt_destroy(ilqr_lqt*) {}
int ilqr_lqt_set_targets(ilqr_lqt*, const double*) { refuse("ilqr_lqt_set_targets"); }
int ilqr_lqt_solve_dp(ilqr_lqt*) { refuse("ilqr_lqt_solve_dp"); }
int ilqr_lqt_solve_lin_al(ilqr_lqt*) { refuse("ilqr_lqt_solve_lin_al"); }
int ilqr_lqt_command(ilqr_lqt*, int, const double*, double*) { refuse("ilqr_lqt_command"); }
int ilqr_lqt_get_U(ilqr_lqt*, double*) { refuse("ilqr_lqt_get_U"); }
int ilqr_lqt_get_X(ilqr_lqt*, double*) { refuse("ilqr_lqt_get_X"); }
}
