// ilqr_steps.hpp -- the step table of a problem's keypoints (HIP-free: the builder is checked on the host by tests/cpp/step_table_main.cpp).
//
// Keypoints may share a timestep (a SequentialSystem whose sub-systems put a keypoint on the same step): their terms add.  The descriptor
// keeps one entry per keypoint, ordered by timestep (within a step by sub-system index, the order of summation); the table lists the
// distinct keypoint steps and, for each, the range of keypoints on it.  With unique timesteps step s is keypoint s.
#pragma once

namespace ilqr {

constexpr int STEP_MAX_KP = 8;  // ILQR_MAX_KP

struct StepTable {
    int n;                     // distinct keypoint steps
    int t[STEP_MAX_KP];        // timestep of step s, strictly ascending
    int kp[STEP_MAX_KP + 1];   // keypoints kp[s] .. kp[s + 1] - 1 sit on step t[s]; kp[n] = the number of keypoints
};

// kp_t[0 .. n_kp) must be non-decreasing and n_kp in 0 .. STEP_MAX_KP; false (and an empty table) otherwise
inline bool build_step_table(const int* kp_t, int n_kp, StepTable& st) {
    st.n = 0;
    for (int s = 0; s < STEP_MAX_KP; s++) st.t[s] = 0;
    for (int s = 0; s <= STEP_MAX_KP; s++) st.kp[s] = 0;
    if (n_kp < 0 || n_kp > STEP_MAX_KP) return false;
    for (int k = 1; k < n_kp; k++)
        if (kp_t[k] < kp_t[k - 1]) return false;
    for (int k = 0; k < n_kp; k++) {
        if (k == 0 || kp_t[k] != kp_t[k - 1]) {
            st.t[st.n] = kp_t[k];
            st.kp[st.n] = k;
            st.n++;
        }
    }
    for (int s = st.n; s <= STEP_MAX_KP; s++) st.kp[s] = n_kp;
    return true;
}

// some step holds more than one keypoint
inline bool has_shared_step(const StepTable& st) { return st.kp[st.n] > st.n; }

}  // namespace ilqr
