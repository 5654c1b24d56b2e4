// mn_obs_noise.hip -- mn_obs_perturb / mn_env_perturb_obs: the observation-noise rule (mn_obs_noise_body.h) on a vector of rows, one launch (gfx950).
// One thread per (row, channel): a channel reads and writes its own one or two elements only, so the launch may run in place.  No LDS; grid-stride, so
// the grid is bounded whatever n.
#include "mn_internal.h"

namespace {

__global__ __launch_bounds__(256) void mn_obs_perturb_kernel(const float *obs_in, float *obs_out, int64_t n, uint64_t env_index0,
                                                             const int32_t *__restrict__ ep_t, MnObsNoiseDev S) {
    const int64_t total = n * MN_OBS_NOISE_CHANNELS, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / MN_OBS_NOISE_CHANNELS;
        const int c = (int)(i - r * MN_OBS_NOISE_CHANNELS);
        const uint64_t key = mn_obs_noise_row_key(S.seed, env_index0 + (uint64_t)r, (uint64_t)(int64_t)ep_t[r]);
        mn_obs_noise_channel(obs_in + r * MN_OBS_DIM, obs_out + r * MN_OBS_DIM, c, key, S);
    }
}

}  // namespace

void mn_launch_obs_perturb(const float *obs_in, float *obs_out, int64_t n, uint64_t env_index0, const int32_t *ep_t, const MnObsNoiseDev &S, hipStream_t s) {
    const int64_t blocks = (n * MN_OBS_NOISE_CHANNELS + 255) / 256;
    hipLaunchKernelGGL(mn_obs_perturb_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, obs_in, obs_out, n, env_index0, ep_t, S);
}
