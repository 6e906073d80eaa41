// ilqr_fwd_io_plan.hpp -- the hand-off protocol of k_forward_reg's helper-wave form (ilqr_kernels_wave.hip, template parameter IO): ring sizes and
// the value each flag word must have reached before each access.  No HIP here: the kernel and tests/cpp/fwd_io_protocol_main.cpp (a host model of
// the waves) both include it, so the model checks the formulas the kernel runs.
//
// Waves of a workgroup: four chain waves (the rollout arithmetic of 4 instances each), a gain loader, an x | u loader and a storer.  Steps are
// n = 0 .. T1 - 1 (T1 = T - 1 control steps).  Everything of step n lives in slot n mod FIO_RING of its ring:
//   gain ring   the 16 gain records of step n as they lie in memory            written by the gain loader, read by the chain waves
//   in ring     xbar | ubar of step n, 14 rows x 16 instances                   written by the x | u loader, read by the chain waves
//   out ring    x(1) | u(1) of step n, 14 rows x 16 instances                   written by the chain waves, read by the storer
// Flag words (counts of steps, written after the data they announce; zero at the start):
//   loaded_g, loaded_v   steps 0 .. loaded - 1 are in the gain ring / the in ring
//   produced[w]          chain wave w has finished steps 0 .. produced[w] - 1: their x(1) | u(1) are in the out ring, and it has read the in ring
//                        of these steps and the gain ring of steps 0 .. produced[w] (a step picks the gains of the next one)
//   stored               the storer has read steps 0 .. stored - 1 out of the out ring
// No cycle of waits: a chain wave ahead of group k0 waits for loads of steps <= k0 + FIO_GROUP and for the store of step
// k0 + FIO_GROUP - 1 - FIO_RING; these wait for every live chain wave to have produced at most k0 + FIO_GROUP + 1 - FIO_RING <= k0 steps (FIO_RING
// > FIO_GROUP), i.e. to have passed a group that starts before k0 -- every chain of waits strictly descends in the group it ends at, and group 0
// waits for loads that wait for nothing.
#pragma once

namespace ilqr {

constexpr int FIO_RING = 8;    // slots of each ring
constexpr int FIO_GROUP = 4;   // steps of a chain wave between two looks at the flags
static_assert(FIO_RING > FIO_GROUP, "the loaders must be able to fill the group ahead of the one the slowest chain wave is in");
static_assert((FIO_RING & (FIO_RING - 1)) == 0 && FIO_RING % FIO_GROUP == 0, "slot = step & (FIO_RING - 1); a group never wraps inside the ring");

constexpr int fio_slot(int n) { return n & (FIO_RING - 1); }
constexpr int fio_min(int a, int b) { return a < b ? a : b; }

// ---- a chain wave, once ahead of the group of steps k0 .. k0 + FIO_GROUP - 1 (k0 a multiple of FIO_GROUP)
// its last step picks the gains of step k0 + FIO_GROUP
constexpr int fio_need_loaded_g(int k0, int T1) { return fio_min(k0 + FIO_GROUP + 1, T1); }
constexpr int fio_need_loaded_v(int k0, int T1) { return fio_min(k0 + FIO_GROUP, T1); }
// it writes the out slots of steps up to k0 + FIO_GROUP - 1, which held the steps FIO_RING earlier (<= 0: nothing to wait for)
constexpr int fio_need_stored(int k0) { return k0 + FIO_GROUP - FIO_RING; }

// ---- a loader, ahead of writing step n into its slot: every live chain wave must have finished step n - FIO_RING (<= 0: nothing to wait for)
constexpr int fio_need_produced_load(int n) { return n + 1 - FIO_RING; }
// ---- the storer, ahead of reading step n out of the out ring: every live chain wave must have finished step n
constexpr int fio_need_produced_store(int n) { return n + 1; }

}  // namespace ilqr
