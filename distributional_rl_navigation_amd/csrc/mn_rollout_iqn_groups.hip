// mn_rollout_iqn_groups.hip -- IQN evaluation episodes of MANY sets of weights in ONE launch (gfx950): mn_rollout_iqn_rows with a weight image and
// a tau stream per group of rows (mn_rollout_iqn_groups; iqn/deferred_eval.py: every pending evaluation point of a training run, or N saved networks).
//
// One launch per set of weights leaves the device idle: an episode workgroup has its CU to itself (the acting weight image fills the LDS), so an
// evaluation on 30 worlds occupies 30 CUs for as long as its longest episode lasts.  Here row e of the handle belongs to group e / rows_per_group; its
// workgroup stages the group's image, reads the group's {seed, counter} and keys its tau draws by e % rows_per_group, so that the group computes -- and
// leaves in its counter and in steps_run[group] -- exactly what mn_rollout_iqn_rows computes on a handle of rows_per_group rows with those worlds,
// that image and that state.  cvar_row / adaptive_row stay indexed by e.
//
// The launch has far more workgroups than CUs, and a group's rows need not be resident together: no workgroup waits for another.  The counter update
// is the body's fire-and-forget ticket, taken in the group's own two words; whoever arrives last in a group writes for it.
//
// The episode itself is iqn_episode<> of mn_rollout_iqn_body.h in its GROUPED form; the contraction rules are written there.
#include "mn_rollout_iqn_body.h"

namespace {

template <typename M, bool PARITY, int L>
__global__ __launch_bounds__(MN_WAVE, 1) void mn_episode_iqn_groups_kernel(MnArrays A, MnDev P, int n_steps, const uint32_t *__restrict__ images, IqnGroups G,
                                                                           uint64_t *rng_states, const float *__restrict__ cvar_row,
                                                                           const uint8_t *__restrict__ adaptive_row, float *__restrict__ obs_io, IqnTrace T,
                                                                           uint32_t *__restrict__ group_words, int32_t *__restrict__ steps_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    iqn_episode<M, PARITY, L, false, true>(lds, A, P, n_steps, images, rng_states, 1.0f, 0, cvar_row, adaptive_row, obs_io, T, group_words, steps_out, G);
}

}  // namespace

void mn_launch_rollout_iqn_groups(const MnArrays &A, const MnDev &P, int precision, int n_steps, const uint32_t *images, int64_t image_stride,
                                  int rows_per_group, uint64_t *rng_states, const float *cvar_row, const uint8_t *adaptive_row, float *obs_io,
                                  float *obs_trace, float *reward_trace, uint8_t *done_trace, uint8_t *info_trace, int32_t *action_trace, float *cvar_trace,
                                  float *q_trace, uint32_t *group_words, int32_t *steps_run, hipStream_t s) {
    const IqnTrace T = {obs_trace, reward_trace, done_trace, info_trace, action_trace, cvar_trace, q_trace, nullptr, nullptr, nullptr};
    const IqnGroups G = {rows_per_group, image_stride};
    constexpr int LL = 8;      // the lane groups of mn_rollout_policy_kernel
    const size_t lds_bytes = IqnLds<false>::FLOATS * sizeof(float);
    if (precision == MN_PRECISION_F64) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_episode_iqn_groups_kernel<double, true, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL((mn_episode_iqn_groups_kernel<double, true, LL>), dim3((unsigned)A.n), dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, images, G, rng_states,
                           cvar_row, adaptive_row, obs_io, T, group_words, steps_run);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_episode_iqn_groups_kernel<float, false, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL((mn_episode_iqn_groups_kernel<float, false, LL>), dim3((unsigned)A.n), dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, images, G, rng_states,
                           cvar_row, adaptive_row, obs_io, T, group_words, steps_run);
    }
}
