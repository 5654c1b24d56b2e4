// replay.hip -- one-launch append of a whole vector step to the device replay ring (gfx950).
//
// Counterpart of ReplayBuffer.add (thirdparty/IQN/replay_buffer.py:26-34) for n transitions at once:
// the reference appends python tuples to a deque(maxlen); here the ring is five HBM tensors in the
// layout sample() hands to the learner (float32 states / next_states [cap][26], int64 actions,
// float32 rewards and dones [cap][1]) and row i of the batch goes to slot (ptr + i) mod cap.
// Pure data movement (~220 B per transition): one coalesced pass instead of ~12 indexed-copy launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "marinenav_hip.h"
#include "iqn_actor_group.h"
#include "dqn_actor_group.h"

namespace {

constexpr int ROW4 = MN_OBS_DIM * 4 / 8;  // 26 floats = 13 float2

__global__ __launch_bounds__(256) void replay_append_kernel(const float2 *__restrict__ obs, const int32_t *__restrict__ actions,
                                                            const float *__restrict__ reward, const float2 *__restrict__ next_obs,
                                                            const uint8_t *__restrict__ done, float2 *__restrict__ r_states,
                                                            float2 *__restrict__ r_next, int64_t *__restrict__ r_actions,
                                                            float *__restrict__ r_rewards, float *__restrict__ r_dones,
                                                            int64_t first, int64_t n, int64_t ptr, int64_t cap) {
    // element index over n * 13 float2 of an observation row block
    const int64_t total = n * ROW4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / ROW4, c = i - row * ROW4;
        int64_t slot = ptr + row;
        slot = slot >= cap ? slot - cap : slot;
        const int64_t src = (first + row) * ROW4 + c;
        r_states[slot * ROW4 + c] = obs[src];
        r_next[slot * ROW4 + c] = next_obs[src];
        if (c == 0) {
            r_actions[slot] = (int64_t)actions[first + row];
            r_rewards[slot] = reward[first + row];
            r_dones[slot] = done[first + row] ? 1.0f : 0.0f;
        }
    }
}

// The n-step window append (marinenav_hip.h, "n-step window"): one pass over k x 13 float2 that stores this call's transition into window slot `wslot` and,
// once the window is full (`emit`), the window's head transition into the ring.  `head` is the oldest slot, (count + 1) % n; `wslot` is count % n: never the
// same for n >= 2, so the head rows read here were written by earlier launches.  Whatever belongs to the newest step -- reward, done, next state -- comes from
// the call's inputs, never from slot `wslot`, which other lanes of the row are writing meanwhile.  Slot i of the age order is (head + i) % n.
// EPISODE: the window is cut at its first done (slot j): return over slots 0..j, next state of slot j, done = any.  Every lane of a row finds j for itself
// (at most n - 1 byte loads of the row's done flags): the row's 13 lanes need it to pick their half of the next state.
template <bool EPISODE>
__global__ __launch_bounds__(256) void replay_append_nstep_kernel(const float2 *__restrict__ obs, const int32_t *__restrict__ actions,
                                                                  const float *__restrict__ reward, const float2 *__restrict__ next_obs,
                                                                  const uint8_t *__restrict__ done, float2 *__restrict__ h_s, int64_t *__restrict__ h_a,
                                                                  float *__restrict__ h_r, float2 *__restrict__ h_ns, uint8_t *__restrict__ h_d,
                                                                  float2 *__restrict__ r_states, float2 *__restrict__ r_next,
                                                                  int64_t *__restrict__ r_actions, float *__restrict__ r_rewards,
                                                                  float *__restrict__ r_dones, const mn_nstep_gamma g, int64_t k, int32_t n, int32_t wslot,
                                                                  int32_t head, int32_t emit, int64_t first, int64_t ptr, int64_t cap) {
#pragma clang fp contract(off)
    const int64_t total = k * ROW4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / ROW4, c = i - row * ROW4;
        const float2 s_new = obs[i], ns_new = next_obs[i];
        const bool d_new = done[row] != 0;
        const int64_t w = (int64_t)wslot * k + row;
        h_s[w * ROW4 + c] = s_new;
        if (EPISODE) h_ns[w * ROW4 + c] = ns_new;
        if (c == 0) {
            h_a[w] = (int64_t)actions[row];
            h_r[w] = reward[row];
            if (EPISODE) h_d[w] = d_new ? 1 : 0;
        }
        if (!emit || row < first) continue;      // window still filling, or a row the ring has no room for (only the newest `cap` rows survive)
        int64_t slot = ptr + (row - first);
        slot = slot >= cap ? slot - cap : slot;
        int32_t j = n - 1;                       // the slot (in age order) the transition ends with
        bool cut = d_new;
        if (EPISODE) {
            int32_t at = head;
            for (int32_t a = 0; a < n - 1; ++a) {
                if (h_d[(int64_t)at * k + row]) { j = a; cut = true; break; }
                at = at + 1 == n ? 0 : at + 1;
            }
        }
        const int64_t hd = (int64_t)head * k + row;
        r_states[slot * ROW4 + c] = h_s[hd * ROW4 + c];
        if (j == n - 1) {
            r_next[slot * ROW4 + c] = ns_new;
        } else {
            int32_t at = head + j;
            at = at >= n ? at - n : at;
            r_next[slot * ROW4 + c] = h_ns[((int64_t)at * k + row) * ROW4 + c];
        }
        if (c == 0) {
            r_actions[slot] = h_a[hd];
            float ret = 0.0f;
            int32_t at = head;
            for (int32_t a = 0; a <= j; ++a) {      // ret = ret + g[a] * r[a]: the product rounds, then the sum (no contraction), first term 0 + x
                const float r = a == n - 1 ? reward[row] : h_r[(int64_t)at * k + row];
                const float term = g.g[a] * r;
                ret = ret + term;
                at = at + 1 == n ? 0 : at + 1;
            }
            r_rewards[slot] = ret;
            r_dones[slot] = cut ? 1.0f : 0.0f;
        }
    }
}

// replay_append_kernel for the G rings of an actor group: rows [g n_group, (g + 1) n_group) of the vector step go to ring g = blockIdx.y, taken from the
// device table by the block's group alone (scalar loads); `n` of a group's rows are stored, from its row `first` on.  Row = the table row of an IQN or a
// DQN actor: both name their ring arrays alike.
template <class Row>
__device__ __forceinline__ void append_group_rows(const Row &r, const float2 *__restrict__ obs, const int32_t *__restrict__ actions,
                                                  const float *__restrict__ reward, const float2 *__restrict__ next_obs,
                                                  const uint8_t *__restrict__ done, int64_t n_group, int64_t first, int64_t n, int64_t ptr, int64_t cap) {
    float2 *__restrict__ r_states = reinterpret_cast<float2 *>(r.ring_states), *__restrict__ r_next = reinterpret_cast<float2 *>(r.ring_next_states);
    const int64_t base = (int64_t)blockIdx.y * n_group + first, total = n * ROW4;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / ROW4, c = i - row * ROW4;
        int64_t slot = ptr + row;
        slot = slot >= cap ? slot - cap : slot;
        const int64_t src = (base + row) * ROW4 + c;
        r_states[slot * ROW4 + c] = obs[src];
        r_next[slot * ROW4 + c] = next_obs[src];
        if (c == 0) {
            r.ring_actions[slot] = (int64_t)actions[base + row];
            r.ring_rewards[slot] = reward[base + row];
            r.ring_dones[slot] = done[base + row] ? 1.0f : 0.0f;
        }
    }
}

__global__ __launch_bounds__(256) void replay_append_groups_kernel(const IqnActorRow *__restrict__ table, const float2 *__restrict__ obs,
                                                                   const int32_t *__restrict__ actions, const float *__restrict__ reward,
                                                                   const float2 *__restrict__ next_obs, const uint8_t *__restrict__ done,
                                                                   int64_t n_group, int64_t first, int64_t n, int64_t ptr, int64_t cap) {
    append_group_rows(table[blockIdx.y], obs, actions, reward, next_obs, done, n_group, first, n, ptr, cap);
}

__global__ __launch_bounds__(256) void replay_append_dqn_groups_kernel(const DqnActorRow *__restrict__ table, const float2 *__restrict__ obs,
                                                                       const int32_t *__restrict__ actions, const float *__restrict__ reward,
                                                                       const float2 *__restrict__ next_obs, const uint8_t *__restrict__ done,
                                                                       int64_t n_group, int64_t first, int64_t n, int64_t ptr, int64_t cap) {
    append_group_rows(table[blockIdx.y], obs, actions, reward, next_obs, done, n_group, first, n, ptr, cap);
}

// the grouped append of a group object of either kind: argument checks, then `kernel` on grid (blocks, G)
template <class Group, class Kernel>
int launch_group_append(Kernel kernel, Group *g, const float *obs_dev, const int32_t *actions_dev, const float *reward_dev, const float *next_obs_dev,
                        const uint8_t *done_dev, int64_t ptr, int64_t capacity, void *stream) {
    if (!g || !g->rings || !obs_dev || !actions_dev || !reward_dev || !next_obs_dev || !done_dev) return MN_ERR_INVALID;
    if (capacity <= 0 || ptr < 0 || ptr >= capacity) return MN_ERR_INVALID;
    int64_t first = 0, n = g->rows;
    if (n > capacity) { first = n - capacity; n = capacity; }   // only the newest `capacity` rows survive (deque maxlen)
    int64_t blocks = (n * ROW4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks, (unsigned)g->n_groups), dim3(256), 0, (hipStream_t)stream, g->table_dev,
                       reinterpret_cast<const float2 *>(obs_dev), actions_dev, reward_dev, reinterpret_cast<const float2 *>(next_obs_dev), done_dev,
                       (int64_t)g->rows, first, n, ptr, capacity);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

}  // namespace

extern "C" int mn_replay_append(const float *obs_dev, const int32_t *actions_dev, const float *reward_dev,
                                const float *next_obs_dev, const uint8_t *done_dev, float *ring_states, float *ring_next_states,
                                int64_t *ring_actions, float *ring_rewards, float *ring_dones, int64_t n, int64_t ptr,
                                int64_t capacity, void *stream) {
    if (!obs_dev || !actions_dev || !reward_dev || !next_obs_dev || !done_dev || !ring_states || !ring_next_states ||
        !ring_actions || !ring_rewards || !ring_dones)
        return MN_ERR_INVALID;
    if (n <= 0 || capacity <= 0 || ptr < 0 || ptr >= capacity) return MN_ERR_INVALID;
    int64_t first = 0;
    if (n > capacity) { first = n - capacity; n = capacity; }   // only the newest `capacity` rows survive (deque maxlen)
    const int64_t total = n * ROW4;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(replay_append_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float2 *>(obs_dev), actions_dev, reward_dev,
                       reinterpret_cast<const float2 *>(next_obs_dev), done_dev, reinterpret_cast<float2 *>(ring_states),
                       reinterpret_cast<float2 *>(ring_next_states), ring_actions, ring_rewards, ring_dones, first, n, ptr, capacity);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

// the n-step window append of k streams (marinenav_hip.h): one launch; the caller counts the window's adds and advances ptr when the call emitted
extern "C" int mn_replay_append_nstep(const float *obs_dev, const int32_t *actions_dev, const float *reward_dev, const float *next_obs_dev,
                                      const uint8_t *done_dev, float *hist_states, int64_t *hist_actions, float *hist_rewards, float *hist_next_states,
                                      uint8_t *hist_dones, int64_t count, int32_t n_step, mn_nstep_gamma gamma_pow, int32_t mode, float *ring_states,
                                      float *ring_next_states, int64_t *ring_actions, float *ring_rewards, float *ring_dones, int64_t k, int64_t ptr,
                                      int64_t capacity, void *stream) {
    if (!obs_dev || !actions_dev || !reward_dev || !next_obs_dev || !done_dev || !hist_states || !hist_actions || !hist_rewards || !ring_states ||
        !ring_next_states || !ring_actions || !ring_rewards || !ring_dones)
        return MN_ERR_INVALID;
    if (mode != MN_NSTEP_REFERENCE && mode != MN_NSTEP_EPISODE) return MN_ERR_INVALID;
    if (mode == MN_NSTEP_EPISODE && (!hist_next_states || !hist_dones)) return MN_ERR_INVALID;
    if (n_step < 2 || n_step > MN_NSTEP_MAX || count < 0) return MN_ERR_INVALID;
    if (k <= 0 || capacity <= 0 || ptr < 0 || ptr >= capacity) return MN_ERR_INVALID;
    const int64_t first = k > capacity ? k - capacity : 0;      // only the newest `capacity` rows survive (deque maxlen)
    const int32_t wslot = (int32_t)(count % n_step), head = (int32_t)((count + 1) % n_step), emit = count + 1 >= n_step;
    int64_t blocks = (k * ROW4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    auto kernel = mode == MN_NSTEP_EPISODE ? replay_append_nstep_kernel<true> : replay_append_nstep_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float2 *>(obs_dev), actions_dev, reward_dev,
                       reinterpret_cast<const float2 *>(next_obs_dev), done_dev, reinterpret_cast<float2 *>(hist_states), hist_actions, hist_rewards,
                       reinterpret_cast<float2 *>(hist_next_states), hist_dones, reinterpret_cast<float2 *>(ring_states),
                       reinterpret_cast<float2 *>(ring_next_states), ring_actions, ring_rewards, ring_dones, gamma_pow, k, n_step, wslot, head, emit, first,
                       ptr, capacity);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

// mn_replay_append for every actor of a group in one launch: row i of group g goes to slot (ptr + i - first) mod capacity of ring g
extern "C" int mn_iqn_actor_group_append(mn_iqn_actor_group *g, const float *obs_dev, const int32_t *actions_dev, const float *reward_dev,
                                         const float *next_obs_dev, const uint8_t *done_dev, int64_t ptr, int64_t capacity, void *stream) {
    return launch_group_append(replay_append_groups_kernel, g, obs_dev, actions_dev, reward_dev, next_obs_dev, done_dev, ptr, capacity, stream);
}

// the same into the rings of a DQN actor group
extern "C" int mn_dqn_actor_group_append(mn_dqn_actor_group *g, const float *obs_dev, const int32_t *actions_dev, const float *reward_dev,
                                         const float *next_obs_dev, const uint8_t *done_dev, int64_t ptr, int64_t capacity, void *stream) {
    return launch_group_append(replay_append_dqn_groups_kernel, g, obs_dev, actions_dev, reward_dev, next_obs_dev, done_dev, ptr, capacity, stream);
}
