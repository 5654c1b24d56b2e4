// mn_rollout_dqn_groups.hip -- DQN evaluation episodes of MANY sets of weights in ONE launch (gfx950): mn_rollout_dqn with a weight image per group
// of rows (mn_rollout_dqn_groups; dqn/deferred_eval.py: every pending evaluation point of a training run, or N saved networks).
//
// One launch per set of weights leaves the device idle: the weight image fills a CU's LDS and a wavefront carries 8 envs, so an evaluation on 30
// worlds is 4 workgroups on 4 CUs for as long as its longest episode lasts.  Here row e of the handle belongs to group e / rows_per_group; a group has
// ceil(rows_per_group / 8) workgroups of its own, each stages the group's image, and the slots of a group's last wavefront behind its last row are
// inactive padding (DqnGroups in mn_rollout_dqn_body.h), so that a group computes exactly what mn_rollout_dqn computes on a handle of rows_per_group
// rows with those worlds and that image.
//
// Workgroups do not communicate: no counters, no tickets, no atomics.  The launch may have more workgroups than CUs; none waits for another.  The
// longest episode of a group is read from the `done` trace on the host.
//
// The episode itself is dqn_episode<> of mn_rollout_dqn_body.h in its GROUPED form; the build flags are written there.
#include "mn_rollout_dqn_body.h"

namespace {

template <typename M, bool PARITY, int L>
__global__ __launch_bounds__(MN_WAVE, 1) void mn_episode_dqn_groups_kernel(MnArrays A, MnDev P, int n_steps, const float *__restrict__ images, DqnGroups G,
                                                                           float *__restrict__ obs_io, DqnTrace T) {
    extern __shared__ __attribute__((aligned(16))) float lds[];          // the group's weight image
    dqn_episode<M, PARITY, L, true>(lds, A, P, n_steps, images, obs_io, T, G);
}

}  // namespace

void mn_launch_rollout_dqn_groups(const MnArrays &A, const MnDev &P, int precision, int n_steps, const float *images, int64_t image_stride, int n_groups,
                                  int rows_per_group, float *obs_io, float *obs_trace, float *reward_trace, uint8_t *done_trace, uint8_t *info_trace,
                                  int32_t *action_trace, float *q_trace, hipStream_t s) {
    const DqnTrace T = {obs_trace, reward_trace, done_trace, info_trace, action_trace, q_trace, nullptr};
    constexpr int LL = 8;
    const int wpg = (rows_per_group + MN_WAVE / LL - 1) / (MN_WAVE / LL);
    const DqnGroups G = {rows_per_group, wpg, image_stride};
    const dim3 grid((unsigned)((int64_t)n_groups * wpg));
    const size_t lds_bytes = IMAGE_FLOATS * sizeof(float);
    if (precision == MN_PRECISION_F64) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_episode_dqn_groups_kernel<double, true, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL((mn_episode_dqn_groups_kernel<double, true, LL>), grid, dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, images, G, obs_io, T);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_episode_dqn_groups_kernel<float, false, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL((mn_episode_dqn_groups_kernel<float, false, LL>), grid, dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, images, G, obs_io, T);
    }
}
