// ilqr_capi_kernels.cpp -- the kernels compiled beside the C-ABI units, and nothing else: the kernels that join instances
// (ilqr_multistart_kernels.hpp), the clearance kernels (ilqr_clearance_kernels.hpp), those of the obstacle terms' cooperative path
// (ilqr_obstacle_coop_kernels.hpp) and, behind them all, those of clearance under the closed-loop covariance (ilqr_cov_clearance_kernels.hpp),
// each for the reason given there.  The includes in front of them, and their order, are those of the unit that
// held these kernels before the C ABI was split by concern: the unit's code object stays what it was, and no edit of host orchestration
// re-emits it.
#include "../../include/ilqr_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ilqr_batchcp.hpp"
#include "ilqr_clearance.hpp"
#include "ilqr_closed_loop.hpp"
#include "ilqr_closed_loop_cov.hpp"
#include "ilqr_ctx.hpp"
#include "ilqr_kernels.hpp"
#include "ilqr_multistart.hpp"
#include "ilqr_obstacle.hpp"
#include "ilqr_plan.hpp"

using namespace ilqr;

// the kernels that join instances (adopt, spread, select, get_at) and their launchers: this is the one translation unit that defines them
#define ILQR_MULTISTART_KERNELS_TU
#include "ilqr_multistart_kernels.hpp"

// the clearance kernels (per state, fold, stats) and their launchers: likewise
#define ILQR_CLEARANCE_KERNELS_TU
#include "ilqr_clearance_kernels.hpp"

// the lane-per-item kernels of the obstacle terms' cooperative path (k_stage_dense, k_obs_ls, k_obs_ls_sum) and their launchers: likewise
#include "ilqr_obstacle_coop_kernels.hpp"

// clearance under the closed-loop covariance (k_cov_clr, k_cov_clr_self, k_cov_clr_fold) and their launchers: likewise, and last, so that every
// kernel in front of them is compiled from the text it was compiled from before
#define ILQR_COV_CLEARANCE_KERNELS_TU
#include "ilqr_cov_clearance_kernels.hpp"
