// mn_rollout_dqn.hip -- DQN evaluation episodes in ONE launch (gfx950): mn_rollout_policy's episode semantics with the DQN baseline's greedy policy.
//
// train_dqn.evaluate and the DQN rows of experiments.run_experiment run one Python iteration per env step (mn_dqn_act, mn_step, half a dozen small
// torch kernels).  Here a wavefront owns EIGHT environments for the whole launch and runs, per step, the network of dqn_qvals_kernel, the argmax and
// MnLane::step: bit-identical to a loop of (mn_dqn_act, mn_step) on the same state.  30 evaluation worlds are 4 workgroups on 4 CUs, 500 sweep worlds 63.
//
// The episode itself is dqn_episode<> of mn_rollout_dqn_body.h in its ungrouped form (one weight image for the launch); the build flags are written there.
#include "mn_rollout_dqn_body.h"

namespace {

template <typename M, bool PARITY, int L>
__global__ __launch_bounds__(MN_WAVE, 1) void mn_rollout_dqn_kernel(MnArrays A, MnDev P, int n_steps, const float *__restrict__ image, float *__restrict__ obs_io,
                                                                    DqnTrace T) {
    extern __shared__ __attribute__((aligned(16))) float lds[];          // the weight image
    dqn_episode<M, PARITY, L, false>(lds, A, P, n_steps, image, obs_io, T, DqnGroups{});
}

// the same episodes on perceived rows (mn_set_obs_noise): dqn_episode<>'s NOISE form
template <typename M, bool PARITY, int L>
__global__ __launch_bounds__(MN_WAVE, 1) void mn_rollout_dqn_noise_kernel(MnArrays A, MnDev P, int n_steps, const float *__restrict__ image,
                                                                          float *__restrict__ obs_io, DqnTrace T, MnObsNoiseArg NS) {
    extern __shared__ __attribute__((aligned(16))) float lds[];          // the weight image
    dqn_episode<M, PARITY, L, false, true>(lds, A, P, n_steps, image, obs_io, T, DqnGroups{}, NS);
}

}  // namespace

void mn_launch_rollout_dqn(const MnArrays &A, const MnDev &P, int precision, int n_steps, const float *image, float *obs_io, float *obs_trace,
                           float *reward_trace, uint8_t *done_trace, uint8_t *info_trace, int32_t *action_trace, float *q_trace, double *traj_trace, hipStream_t s,
                           const MnObsNoiseDev *noise, uint64_t noise_env0) {
    const DqnTrace T = {obs_trace, reward_trace, done_trace, info_trace, action_trace, q_trace, traj_trace};
    constexpr int LL = 8;
    const dim3 grid((unsigned)((A.n + MN_WAVE / LL - 1) / (MN_WAVE / LL)));      // (npad is a multiple of 256: the last wave's idle lane groups load padding)
    const size_t lds_bytes = IMAGE_FLOATS * sizeof(float);
    if (noise) {
        const MnObsNoiseArg NS = {*noise, noise_env0};
        if (precision == MN_PRECISION_F64) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_rollout_dqn_noise_kernel<double, true, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            hipLaunchKernelGGL((mn_rollout_dqn_noise_kernel<double, true, LL>), grid, dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, image, obs_io, T, NS);
        } else {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_rollout_dqn_noise_kernel<float, false, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            hipLaunchKernelGGL((mn_rollout_dqn_noise_kernel<float, false, LL>), grid, dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, image, obs_io, T, NS);
        }
        return;
    }
    if (precision == MN_PRECISION_F64) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_rollout_dqn_kernel<double, true, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL((mn_rollout_dqn_kernel<double, true, LL>), grid, dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, image, obs_io, T);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_rollout_dqn_kernel<float, false, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL((mn_rollout_dqn_kernel<float, false, LL>), grid, dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, image, obs_io, T);
    }
}
