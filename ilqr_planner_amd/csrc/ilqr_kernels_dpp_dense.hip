// ilqr_kernels_dpp_dense.hip -- the dense instantiations of k_backward_si_dpp (IO = SW_DENSE: a problem with obstacle terms on the cooperative
// path, RiccatiPlan::obs_dense) and their launcher, in a code object of their own: the kernel's text is ilqr_kernels_dpp.hip, which says why.
#define ILQR_DPP_DENSE_TU
#include "ilqr_kernels_dpp.hip"
