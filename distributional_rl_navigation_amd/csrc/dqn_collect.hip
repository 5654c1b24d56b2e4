// dqn_collect.hip -- the collect phase of DQN training on the device (gfx950): the epsilon-greedy act of a whole vector of environments in ONE
// launch, and the same for the G actors of a group (the seeds of one config, stacked in one env handle) with the actor as the second grid dimension.
//
// DQNAgent.act_batch (dqn/agent.py) is the greedy policy of dqn_act.hip followed by three eager PyTorch launches that draw the exploration from a
// torch.Generator.  Here row e of call number `ctr` under `seed` draws u_e = u01(e, draw_keys(seed, ctr)) -- the counter-based generator of the IQN act
// kernels (iqn_act_common.h; host twin: tests/rng_twin.py, tests/dqn_rng_twin.py) -- and the IQN epilogue's rule decides: greedy iff u > eps, else
// min((int)(u / eps * 9.0f), 8); !(eps > 0): greedy everywhere.  Seed and call number are kernel arguments: no generator state lives on the device.
//   * the greedy action is dqn_argmax(dqn_forward(...)) of dqn_net.h on the weight image in LDS, one wavefront per tile of 16 rows, exactly as
//     dqn_qvals_kernel runs it: a column of the C tile depends on its own column of B only, so a row's Q-values and greedy action are mn_dqn_act's bits;
//   * without a Q-value output only the rows that do not explore need the network: a wavefront whose tile has none skips the forward (a wave-uniform
//     branch), and a workgroup none of whose tiles has one does not copy the 125-KB image into LDS -- decided by a block-wide vote in front of the copy,
//     so every thread takes the same side of the barrier;
//   * the grouped kernels take everything an actor owns from a device table indexed by blockIdx.y alone (scalar loads), and the call numbers from the
//     argument block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "mn_internal.h"
#include "dqn_actor_group.h"

namespace {

#include "dqn_net.h"

// the draws of iqn_act_common.h (that header and dqn_net.h both name the network's widths, so it cannot be included beside it)
__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ float u01(uint32_t idx, uint32_t k0, uint32_t k1) {      // 24-bit uniform in [0, 1)
    return (float)(fmix32(fmix32(idx ^ k0) + k1) >> 8) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ void draw_keys(uint64_t seed, uint64_t ctr, uint32_t &k0, uint32_t &k1) {
    const uint64_t base = mix64(seed + 0x9E3779B97F4A7C15ull * (ctr + 1));
    k0 = (uint32_t)base; k1 = (uint32_t)(base >> 32);
}
__device__ __forceinline__ int explore_action(float u, float eps) {
    const int act = (int)(u / eps * (float)A);
    return act > A - 1 ? A - 1 : act;
}

// Rows [0, n) of one actor: obs [n][26], image = its weight image (global), lds = the workgroup's IMAGE_FLOATS floats.  Workgroup blockIdx.x of
// gridDim.x; what is written does not depend on gridDim.x.
__device__ __forceinline__ void act_rows(const float *__restrict__ obs, const float *__restrict__ image, uint64_t seed, uint64_t ctr, float eps,
                                         float *__restrict__ explore_u, float *__restrict__ qvals, int32_t *__restrict__ actions, int n, float *lds) {
    const int lane = threadIdx.x & 63, g = lane >> 4, col = lane & 15, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int n_tiles = (n + 15) / 16;
    const bool explore = eps > 0.f;
    uint32_t k0, k1;
    draw_keys(seed, ctr, k0, k1);
    bool stage = qvals != nullptr;      // block-uniform: with a Q-value output every row is evaluated
    if (!stage) {
        bool need = false;
        for (int tile = blockIdx.x * waves + wave; tile < n_tiles; tile += gridDim.x * waves) {
            const int e = tile * 16 + col;
            need = need || (e < n && (!explore || u01((uint32_t)e, k0, k1) > eps));
        }
        int *flags = reinterpret_cast<int *>(lds);
        const bool wave_need = __ballot(need) != 0ull;
        if (lane == 0) flags[wave] = wave_need ? 1 : 0;
        __syncthreads();
        int any = 0;
        for (int w = 0; w < waves; ++w) any |= flags[w];
        __syncthreads();      // (the copy below overwrites the flags)
        stage = any != 0;
    }
    if (stage) {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(image);
        f32x4 *dst = reinterpret_cast<f32x4 *>(lds);
        for (int i = threadIdx.x; i < IMAGE_FLOATS / 4; i += blockDim.x) dst[i] = src[i];
        __syncthreads();
    }
    for (int tile = blockIdx.x * waves + wave; tile < n_tiles; tile += gridDim.x * waves) {
        const int e = tile * 16 + col;
        const bool live = e < n;
        const float u = u01((uint32_t)e, k0, k1);
        const bool greedy = !explore || u > eps;
        if (explore_u && live && g == 0) explore_u[e] = u;
        int arg = 0;
        if (qvals != nullptr || __ballot(live && greedy) != 0ull) {      // wave-uniform
            // observation row of env `col`, features 16 t + 4 g + r (26 inputs, zero-padded to 32)
            f32x4 x0[2];
            const float *row = obs + (size_t)(live ? e : 0) * OBS;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = 16 * t + 4 * g + r;
                    x0[t][r] = (live && k < OBS) ? row[k < OBS ? k : 0] : 0.f;
                }
            const f32x4 q = dqn_forward(lds, lane, x0);
            if (qvals && live)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * g + r < A) qvals[(size_t)e * A + 4 * g + r] = q[r];
            arg = dqn_argmax(q, g);
        }
        if (live && g == 0) actions[e] = greedy ? arg : explore_action(u, eps);
    }
}

__global__ __launch_bounds__(512) void dqn_act_rng_kernel(const float *__restrict__ obs, const float *__restrict__ image, uint64_t seed, uint64_t ctr,
                                                          float eps, float *__restrict__ explore_u, float *__restrict__ qvals,
                                                          int32_t *__restrict__ actions, int n) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    act_rows(obs, image, seed, ctr, eps, explore_u, qvals, actions, n, lds);
}

struct CallIndices { uint64_t v[MN_DQN_MAX_ACTORS]; };      // travels in the argument block

// actor blockIdx.y on rows [y n, (y + 1) n) of the stacked obs / actions; the draw's index is the row inside the group
__global__ __launch_bounds__(512) void dqn_group_act_rng_kernel(const DqnActorRow *__restrict__ table, const float *__restrict__ obs, float eps,
                                                                const CallIndices calls, int32_t *__restrict__ actions, int n) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const DqnActorRow &r = table[blockIdx.y];
    const size_t first = (size_t)blockIdx.y * n;
    act_rows(obs + first * OBS, r.image, r.seed, calls.v[blockIdx.y], eps, nullptr, nullptr, actions + first, n, lds);
}

// W_l[out][in] of layer l with the encoders as one block-diagonal [208][32] matrix; zero outside the true shape.  The image layout and these two
// functions are dqn_act.hip's (dqn_pack_kernel): element i of an image is a copy of one weight or a zero, so both packs write the same bytes.
__device__ __forceinline__ float layer_weight(const float *const *w, int l, int out, int in) {
    switch (l) {
        case 0:
            if (out < 16) return in < 2 ? w[0][out * 2 + in] : 0.f;
            if (out < 32) return (in >= 2 && in < 4) ? w[2][(out - 16) * 2 + (in - 2)] : 0.f;
            return (out < F && in >= 4 && in < OBS) ? w[4][(out - 32) * 22 + (in - 4)] : 0.f;
        case 1: return (out < H && in < F) ? w[6][out * F + in] : 0.f;
        case 2: return (out < H && in < H) ? w[8][out * H + in] : 0.f;
        case 3: return (out < A && in < H) ? w[10][out * H + in] : 0.f;
        case 4: return (out < H && in < A) ? w[12][out * A + in] : 0.f;
        case 5: return (out < H && in < H) ? w[14][out * H + in] : 0.f;
        default: return (out < A && in < H) ? w[16][out * H + in] : 0.f;
    }
}
__device__ __forceinline__ float layer_bias(const float *const *w, int l, int out) {
    switch (l) {
        case 0: return out < 16 ? w[1][out] : (out < 32 ? w[3][out - 16] : (out < F ? w[5][out - 32] : 0.f));
        case 1: return out < H ? w[7][out] : 0.f;
        case 2: return out < H ? w[9][out] : 0.f;
        case 3: return out < A ? w[11][out] : 0.f;
        case 4: return out < H ? w[13][out] : 0.f;
        case 5: return out < H ? w[15][out] : 0.f;
        default: return out < A ? w[17][out] : 0.f;
    }
}

// dqn_pack_kernel for the actors of a group whose bit of `stale` is set: image[lw_off(l) + ((mt KT + t) 64 + lane) 4 + r] =
// W_l[16 mt + (lane & 15)][16 t + 4 (lane >> 4) + r], then the biases
__global__ __launch_bounds__(256) void dqn_group_pack_kernel(const DqnActorRow *__restrict__ table, uint64_t stale) {
    if (!((stale >> blockIdx.y) & 1ull)) return;
    const DqnActorRow &a = table[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= IMAGE_FLOATS) return;
    if (i >= OFF_BIAS) {
        int l = 0, k = i - OFF_BIAS;
        while (k >= LM[l] * 16) { k -= LM[l] * 16; ++l; }
        a.image[i] = layer_bias(a.weights, l, k);
        return;
    }
    int l = 0, k = i;
    while (k >= LM[l] * LK[l] * 256) { k -= LM[l] * LK[l] * 256; ++l; }
    const int r = k & 3, lane = (k >> 2) & 63, q = k >> 8, t = q % LK[l], mt = q / LK[l];
    a.image[i] = layer_weight(a.weights, l, 16 * mt + (lane & 15), 16 * t + 4 * (lane >> 4) + r);
}

// the act kernels' dynamic LDS limit, once per device
int set_lds_limit(int dev) {
    static bool attr_set[64] = {false};
    if (dev < 0 || dev >= 64) return MN_ERR_NO_DEVICE;
    if (attr_set[dev]) return MN_OK;
    for (const void *k : {reinterpret_cast<const void *>(dqn_act_rng_kernel), reinterpret_cast<const void *>(dqn_group_act_rng_kernel)})
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, IMAGE_FLOATS * (int)sizeof(float)) != hipSuccess) return MN_ERR_HIP;
    attr_set[dev] = true;
    return MN_OK;
}

}  // namespace

extern "C" int mn_dqn_act_rng(const float *obs_dev, const float *const *weights, float *image_dev, int32_t repack, uint64_t seed, uint64_t call_index,
                              float eps, float *explore_u_dev, float *qvals_dev, int32_t *actions_dev, int32_t n, void *stream) {
    if (!obs_dev || !weights || !image_dev || !actions_dev || n <= 0) return MN_ERR_INVALID;
    for (int i = 0; i < 18; ++i) if (!weights[i]) return MN_ERR_INVALID;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || hipGetDeviceProperties(&prop, dev) != hipSuccess) return MN_ERR_NO_DEVICE;
    if (const int rc = set_lds_limit(dev)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (repack) mn_launch_dqn_pack(weights, image_dev, s);
    const int n_tiles = (n + 15) / 16;
    int blocks = (n_tiles + 7) / 8;
    if (blocks > prop.multiProcessorCount) blocks = prop.multiProcessorCount;
    hipLaunchKernelGGL(dqn_act_rng_kernel, dim3(blocks), dim3(512), IMAGE_FLOATS * sizeof(float), s, obs_dev, (const float *)image_dev, seed, call_index,
                       eps, explore_u_dev, qvals_dev, actions_dev, n);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

extern "C" int mn_dqn_actor_group_create(const mn_dqn_actor *actors_host, int32_t n_actors, int32_t rows_per_group, mn_dqn_actor_group **out) {
    if (!out) return MN_ERR_INVALID;
    *out = nullptr;
    if (!actors_host || n_actors < 1 || n_actors > MN_DQN_MAX_ACTORS || rows_per_group < 1) return MN_ERR_INVALID;
    bool rings = true;
    for (int g = 0; g < n_actors; ++g) {
        const mn_dqn_actor &a = actors_host[g];
        if (!a.weights || !a.image) return MN_ERR_INVALID;
        for (int i = 0; i < 18; ++i) if (!a.weights[i]) return MN_ERR_INVALID;
        const void *ring[5] = {a.ring_states, a.ring_next_states, a.ring_actions, a.ring_rewards, a.ring_dones};
        int given = 0;
        for (const void *p : ring) given += p != nullptr;
        if (given != 0 && given != 5) return MN_ERR_INVALID;
        rings = rings && given == 5;
        // actors that alias would race silently: nothing one actor writes may be what another writes
        for (int h = 0; h < g; ++h) {
            const mn_dqn_actor &b = actors_host[h];
            if (a.image == b.image) return MN_ERR_INVALID;
            const void *other[5] = {b.ring_states, b.ring_next_states, b.ring_actions, b.ring_rewards, b.ring_dones};
            for (const void *p : ring)
                for (const void *q : other)
                    if (p && p == q) return MN_ERR_INVALID;
        }
    }
    if (!rings)      // (a group that only ever acts has no ring at all)
        for (int g = 0; g < n_actors; ++g)
            if (actors_host[g].ring_states) return MN_ERR_INVALID;
    int dev = -1;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return MN_ERR_NO_DEVICE;
    if (const int rc = set_lds_limit(dev)) return rc;
    mn_dqn_actor_group *grp = new mn_dqn_actor_group{};
    grp->n_groups = n_actors; grp->rows = rows_per_group; grp->device = dev; grp->n_cu = prop.multiProcessorCount; grp->rings = rings;
    std::vector<DqnActorRow> table(n_actors);
    for (int g = 0; g < n_actors; ++g) {
        const mn_dqn_actor &a = actors_host[g];
        DqnActorRow &r = table[g];
        for (int i = 0; i < 18; ++i) r.weights[i] = a.weights[i];
        r.image = a.image; r.seed = a.seed;
        r.ring_states = a.ring_states; r.ring_next_states = a.ring_next_states; r.ring_actions = a.ring_actions;
        r.ring_rewards = a.ring_rewards; r.ring_dones = a.ring_dones;
    }
    if (hipMalloc(reinterpret_cast<void **>(&grp->table_dev), sizeof(DqnActorRow) * n_actors) != hipSuccess ||
        hipMemcpy(grp->table_dev, table.data(), sizeof(DqnActorRow) * n_actors, hipMemcpyHostToDevice) != hipSuccess) {
        if (grp->table_dev) (void)hipFree(grp->table_dev);
        delete grp;
        return MN_ERR_HIP;
    }
    *out = grp;
    return MN_OK;
}

extern "C" int mn_dqn_actor_group_destroy(mn_dqn_actor_group *g) {
    if (!g) return MN_ERR_INVALID;
    const hipError_t e = hipFree(g->table_dev);
    delete g;
    return e == hipSuccess ? MN_OK : MN_ERR_HIP;
}

extern "C" int mn_dqn_actor_group_set_grid(mn_dqn_actor_group *g, int32_t workgroups_per_group) {
    if (!g || workgroups_per_group < 0) return MN_ERR_INVALID;
    g->grid = workgroups_per_group;
    return MN_OK;
}

extern "C" int mn_dqn_actor_group_act(mn_dqn_actor_group *g, const float *obs_dev, float eps, uint64_t stale_mask, const uint64_t *call_index_host,
                                      int32_t *actions_dev, void *stream) {
    if (!g || !obs_dev || !call_index_host || !actions_dev) return MN_ERR_INVALID;
    if (g->n_groups < 64 && (stale_mask >> g->n_groups) != 0) return MN_ERR_INVALID;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != g->device) return MN_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (stale_mask)
        hipLaunchKernelGGL(dqn_group_pack_kernel, dim3((IMAGE_FLOATS + 255) / 256, (unsigned)g->n_groups), dim3(256), 0, s,
                           (const DqnActorRow *)g->table_dev, stale_mask);
    // Workgroups per group.  Every workgroup with a greedy row copies the 125-KB image into LDS, one workgroup per CU at a time: G x ceil(tiles / 8)
    // workgroups can be several rounds of CUs that each pay that copy again, so a group gets its share of the CUs (results do not depend on the count).
    const int n_tiles = (g->rows + 15) / 16;
    int blocks = (n_tiles + 7) / 8;
    const int cap = g->grid > 0 ? g->grid : (g->n_cu / g->n_groups > 1 ? g->n_cu / g->n_groups : 1);
    if (blocks > cap) blocks = cap;
    CallIndices calls = {};
    for (int i = 0; i < g->n_groups; ++i) calls.v[i] = call_index_host[i];
    hipLaunchKernelGGL(dqn_group_act_rng_kernel, dim3((unsigned)blocks, (unsigned)g->n_groups), dim3(512), IMAGE_FLOATS * sizeof(float), s,
                       (const DqnActorRow *)g->table_dev, obs_dev, eps, calls, actions_dev, g->rows);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}
