// mn_rollout_iqn.hip -- IQN evaluation episodes in ONE launch (gfx950): mn_rollout_policy's episode semantics with the learned policy.
//
// IQNAgent.evaluation_vec runs one Python iteration per env step (act launches, step launch, ~20 small torch kernels, one host
// round trip).  Here a wavefront owns ONE environment for the whole launch and, per step, computes exactly what one mn_iqn_act_rng call
// at eps = 0 computes for that row -- the call's per-row taus (draw_keys / tau_draw of call counter counter0 + t, cvar scalar or
// adjust_cvar of the row), the split-f16 network of iqn_qvals_split_kernel on the row (same device functions, same arithmetic), mean over
// the taus, argmax with the first maximum winning -- then the same MnLane::step as mn_rollout_policy_kernel.  Bit-identical to a loop of
// (mn_iqn_act_rng, mn_step) on the same state, the act call counter included: it ends at counter0 + steps_run, steps_run = the longest
// episode of the launch (the loop acts once per step while any env is alive).
// The cvar and the adaptive flag are the launch's scalars or, for the experiment sweep's five IQN policies side by side in one handle, per env
// (mn_rollout_iqn_rows): the taus are keyed by the env index, so that launch draws what the sweep's one act call on all rows draws.
//
// One wavefront per workgroup (the step's sonar work-list is workgroup LDS), and the acting weight image (sp::ACT_IMG_FLOATS) fills the CU's LDS, so
// a workgroup has its CU to itself.  All eight 8-lane groups of the wave load the same environment so that every value the step
// computes is valid; group 0 alone is `active` (writes rows, traces, the pose).
//
// The episode itself is iqn_episode<> of mn_rollout_iqn_body.h, which mn_rollout_iqn_eval.hip instantiates in act_eval's form (quantile and tau traces); the
// contraction rules of both files are written there.
#include "mn_rollout_iqn_body.h"

namespace {

template <typename M, bool PARITY, int L>
__global__ __launch_bounds__(MN_WAVE, 1) void mn_rollout_iqn_kernel(MnArrays A, MnDev P, int n_steps, const uint32_t *__restrict__ packed,
                                                                    uint64_t *rng_state, float cvar, int adaptive, const float *__restrict__ cvar_row,
                                                                    const uint8_t *__restrict__ adaptive_row, float *__restrict__ obs_io, IqnTrace T,
                                                                    uint32_t *__restrict__ words, int32_t *__restrict__ steps_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    iqn_episode<M, PARITY, L, false>(lds, A, P, n_steps, packed, rng_state, cvar, adaptive, cvar_row, adaptive_row, obs_io, T, words, steps_out,
                                     IqnGroups{});      // one group: the whole launch
}

// the same episodes on perceived rows (mn_set_obs_noise): iqn_episode<>'s NOISE form, one more row of LDS
template <typename M, bool PARITY, int L>
__global__ __launch_bounds__(MN_WAVE, 1) void mn_rollout_iqn_noise_kernel(MnArrays A, MnDev P, int n_steps, const uint32_t *__restrict__ packed,
                                                                          uint64_t *rng_state, float cvar, int adaptive, const float *__restrict__ cvar_row,
                                                                          const uint8_t *__restrict__ adaptive_row, float *__restrict__ obs_io, IqnTrace T,
                                                                          uint32_t *__restrict__ words, int32_t *__restrict__ steps_out, MnObsNoiseArg NS) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    iqn_episode<M, PARITY, L, false, false, true>(lds, A, P, n_steps, packed, rng_state, cvar, adaptive, cvar_row, adaptive_row, obs_io, T, words, steps_out,
                                                  IqnGroups{}, NS);
}

}  // namespace

void mn_launch_rollout_iqn_rows(const MnArrays &A, const MnDev &P, int precision, int n_steps, const uint32_t *image, uint64_t *rng_state, float cvar,
                                int adaptive, const float *cvar_row, const uint8_t *adaptive_row, float *obs_io, float *obs_trace, float *reward_trace,
                                uint8_t *done_trace, uint8_t *info_trace, int32_t *action_trace, float *cvar_trace, float *q_trace, double *traj_trace,
                                uint32_t *words, int32_t *steps_run, hipStream_t s, const MnObsNoiseDev *noise, uint64_t noise_env0) {
    const IqnTrace T = {obs_trace, reward_trace, done_trace, info_trace, action_trace, cvar_trace, q_trace, traj_trace, nullptr, nullptr};
    constexpr int LL = 8;      // the lane groups of mn_rollout_policy_kernel
    if (noise) {
        const MnObsNoiseArg NS = {*noise, noise_env0};
        const size_t bytes = IqnLds<false, true>::FLOATS * sizeof(float);
        if (precision == MN_PRECISION_F64) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_rollout_iqn_noise_kernel<double, true, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            hipLaunchKernelGGL((mn_rollout_iqn_noise_kernel<double, true, LL>), dim3((unsigned)A.n), dim3(MN_WAVE), bytes, s, A, P, n_steps, image, rng_state, cvar,
                               adaptive, cvar_row, adaptive_row, obs_io, T, words, steps_run, NS);
        } else {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_rollout_iqn_noise_kernel<float, false, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            hipLaunchKernelGGL((mn_rollout_iqn_noise_kernel<float, false, LL>), dim3((unsigned)A.n), dim3(MN_WAVE), bytes, s, A, P, n_steps, image, rng_state, cvar,
                               adaptive, cvar_row, adaptive_row, obs_io, T, words, steps_run, NS);
        }
        return;
    }
    const size_t lds_bytes = IqnLds<false>::FLOATS * sizeof(float);
    if (precision == MN_PRECISION_F64) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_rollout_iqn_kernel<double, true, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL((mn_rollout_iqn_kernel<double, true, LL>), dim3((unsigned)A.n), dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, image, rng_state, cvar,
                           adaptive, cvar_row, adaptive_row, obs_io, T, words, steps_run);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_rollout_iqn_kernel<float, false, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL((mn_rollout_iqn_kernel<float, false, LL>), dim3((unsigned)A.n), dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, image, rng_state, cvar,
                           adaptive, cvar_row, adaptive_row, obs_io, T, words, steps_run);
    }
}
