// mn_episode_log.hip -- the per-episode training record of a vector step in ONE launch, without a host look (gfx950).
//
// Counterpart of the block the reference prints at every training episode end (thirdparty/IQN/agent.py:118-119, 152-168: length,
// discounted return, result, exploration rate, timestep) for n envs stepped side by side.  Per env, in float64, every operation
// rounding on its own (the object is built with -ffp-contract=off):
//     ret += disc * (double)reward;   disc *= discount;   len += 1
// and where `done` is set the env writes ONE record (step_index, env, len, info, ret, eps) and goes back to (0, 1, 0).
// The discount factor of a step is the RUNNING PRODUCT discount * discount * ... -- the documented form of this record's return; it
// is not the reference's power `discount ** ep_length` (pow() differs from it in the last bits).
//
// Compaction: each wavefront ballots its finished lanes, one lane claims popcount slots with a single relaxed agent-scope atomic add
// on the counter, each finished lane writes at base + its rank among the finished lanes.  A slot at or beyond `capacity` is not
// written and the counter keeps counting: count - capacity is the exact number of dropped records.  Nothing waits for another
// workgroup, no LDS, plain vector stores; the order of the records of one call is unspecified (episode_log.py sorts).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "marinenav_hip.h"

namespace {

constexpr int EPLOG_BLOCK = 256;

__global__ __launch_bounds__(EPLOG_BLOCK) void mn_episode_log_kernel(const float *__restrict__ reward, const uint8_t *__restrict__ done,
                                                                     const uint8_t *__restrict__ info, int32_t n, double discount,
                                                                     int64_t step_index, float eps, double *__restrict__ ep_ret,
                                                                     double *__restrict__ ep_disc, int32_t *__restrict__ ep_len,
                                                                     int64_t *__restrict__ rec_step, int32_t *__restrict__ rec_env,
                                                                     int32_t *__restrict__ rec_len, uint8_t *__restrict__ rec_info,
                                                                     double *__restrict__ rec_ret, float *__restrict__ rec_eps,
                                                                     int64_t capacity, uint32_t *__restrict__ count) {
    const int32_t i = (int32_t)(blockIdx.x * EPLOG_BLOCK + threadIdx.x);      // (n <= 2^31 - 1 and the grid covers it once)
    const bool live = i < n;
    double ret = 0.0;
    int32_t len = 0;
    bool fin = false;
    if (live) {
        const double disc = ep_disc[i];
        ret = ep_ret[i] + disc * (double)reward[i];
        len = ep_len[i] + 1;
        fin = done[i] != 0;
        ep_ret[i] = fin ? 0.0 : ret;
        ep_disc[i] = fin ? 1.0 : disc * discount;
        ep_len[i] = fin ? 0 : len;
    }
    // every lane of the wavefront reaches the ballot (lanes past n vote false)
    const unsigned long long mask = __ballot(fin);
    if (mask == 0ull) return;
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if (lane == leader) base = __hip_atomic_fetch_add(count, (uint32_t)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = (uint32_t)__shfl((int)base, leader);
    if (!fin) return;
    const int64_t slot = (int64_t)base + (int64_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (slot >= capacity) return;
    rec_step[slot] = step_index;
    rec_env[slot] = i;
    rec_len[slot] = len;
    rec_info[slot] = info[i];
    rec_ret[slot] = ret;
    rec_eps[slot] = eps;
}

}  // namespace

extern "C" int mn_episode_log(const float *reward_dev, const uint8_t *done_dev, const uint8_t *info_dev, int32_t n, double discount,
                              int64_t step_index, float eps, double *ep_ret_dev, double *ep_disc_dev, int32_t *ep_len_dev,
                              int64_t *rec_step, int32_t *rec_env, int32_t *rec_len, uint8_t *rec_info, double *rec_ret, float *rec_eps,
                              int64_t capacity, uint32_t *count_dev, void *stream) {
    if (!reward_dev || !done_dev || !info_dev || !ep_ret_dev || !ep_disc_dev || !ep_len_dev || !count_dev) return MN_ERR_INVALID;
    if (n <= 0 || capacity < 0) return MN_ERR_INVALID;
    if (capacity > 0 && (!rec_step || !rec_env || !rec_len || !rec_info || !rec_ret || !rec_eps)) return MN_ERR_INVALID;
    const unsigned blocks = (unsigned)(((int64_t)n + EPLOG_BLOCK - 1) / EPLOG_BLOCK);
    hipLaunchKernelGGL(mn_episode_log_kernel, dim3(blocks), dim3(EPLOG_BLOCK), 0, (hipStream_t)stream, reward_dev, done_dev, info_dev, n,
                       discount, step_index, eps, ep_ret_dev, ep_disc_dev, ep_len_dev, rec_step, rec_env, rec_len, rec_info, rec_ret,
                       rec_eps, capacity, count_dev);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}
