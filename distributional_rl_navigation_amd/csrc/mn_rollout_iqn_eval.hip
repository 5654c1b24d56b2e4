// mn_rollout_iqn_eval.hip -- IQN evaluation episodes in ONE launch, acting as IQNAgent.act_eval does and recording what each action was chosen
// from (gfx950): mn_rollout_iqn_rows plus the quantile and tau traces (mn_rollout_iqn_eval; the experiment sweep's captured episodes).
//
// Same episode as mn_rollout_iqn.hip (iqn_episode<> of mn_rollout_iqn_body.h, one wavefront per environment), in the QUANT = true form of
// iqn_qvals_split_kernel: the output layer runs per tau on the matrix pipe (q_quantiles, iqn_act_split.h -- the device function that kernel calls),
// Q is the mean of those values and the first maximum wins.  Per step bit-identical to one mn_iqn_act_rng call with quantiles_dev != NULL at eps = 0
// on the row, then mn_step.  The acting form takes the tau mean in front of the output layer; the two can differ in the last bit, which is why this is a
// kernel of its own and not a flag of the acting one.
//
// LDS: the full weight image up to sp::OFF_FB -- incl. the output layer's MFMA operands at OFF_W4H, which the acting image leaves out --, behind it one
// feature buffer and the observation row (IqnLds<true>): 4 KB more than the acting episode kernel, inside the CU's 160 KB.
#include "mn_rollout_iqn_body.h"

namespace {

template <typename M, bool PARITY, int L>
__global__ __launch_bounds__(MN_WAVE, 1) void mn_episode_iqn_eval_kernel(MnArrays A, MnDev P, int n_steps, const uint32_t *__restrict__ packed,
                                                                         uint64_t *rng_state, float cvar, int adaptive, const float *__restrict__ cvar_row,
                                                                         const uint8_t *__restrict__ adaptive_row, float *__restrict__ obs_io, IqnTrace T,
                                                                         uint32_t *__restrict__ words, int32_t *__restrict__ steps_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    iqn_episode<M, PARITY, L, true>(lds, A, P, n_steps, packed, rng_state, cvar, adaptive, cvar_row, adaptive_row, obs_io, T, words, steps_out,
                                     IqnGroups{});      // one group: the whole launch
}

}  // namespace

void mn_launch_rollout_iqn_eval(const MnArrays &A, const MnDev &P, int precision, int n_steps, const uint32_t *image, uint64_t *rng_state, float cvar,
                                int adaptive, const float *cvar_row, const uint8_t *adaptive_row, float *obs_io, float *obs_trace, float *reward_trace,
                                uint8_t *done_trace, uint8_t *info_trace, int32_t *action_trace, float *cvar_trace, float *q_trace, double *traj_trace,
                                float *quantiles_trace, float *taus_trace, uint32_t *words, int32_t *steps_run, hipStream_t s) {
    const IqnTrace T = {obs_trace, reward_trace, done_trace, info_trace, action_trace, cvar_trace, q_trace, traj_trace, quantiles_trace, taus_trace};
    constexpr int LL = 8;      // the lane groups of mn_rollout_policy_kernel
    const size_t lds_bytes = IqnLds<true>::FLOATS * sizeof(float);
    if (precision == MN_PRECISION_F64) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_episode_iqn_eval_kernel<double, true, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL((mn_episode_iqn_eval_kernel<double, true, LL>), dim3((unsigned)A.n), dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, image, rng_state, cvar,
                           adaptive, cvar_row, adaptive_row, obs_io, T, words, steps_run);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_episode_iqn_eval_kernel<float, false, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL((mn_episode_iqn_eval_kernel<float, false, LL>), dim3((unsigned)A.n), dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, image, rng_state, cvar,
                           adaptive, cvar_row, adaptive_row, obs_io, T, words, steps_run);
    }
}
