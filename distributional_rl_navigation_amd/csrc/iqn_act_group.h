// iqn_act_group.h -- the act call of MANY actors in one launch each (mn_iqn_actor_group_act): the preparation and act kernels of iqn_act_split.h with the
// group as the second grid dimension.  Group g is rows [g n, (g + 1) n) of the launch's observations and actions and row g of the device table
// (IqnActorRow: its network, weight image, constants, generator state, draws and greedy-row list).  Every kernel body here is the single call's own --
// split_consts_block, pack_word, draw_block, iqn_act_split_body.h -- and addresses its rows through blockIdx.x / gridDim.x, which in an (X, G) grid are
// the values of a launch of that group alone: workgroup (w, g) is workgroup w of group g's single call on n rows.  Included by iqn_act.hip only.

namespace sp {

__device__ __forceinline__ IqnWeights actor_weights(const IqnActorRow &r) {
    return IqnWeights{r.weights[0], r.weights[1], r.weights[2], r.weights[3], r.weights[4], r.weights[5], r.weights[6],
                      r.weights[7], r.weights[8], r.weights[9], r.weights[10], r.weights[11], r.weights[12], r.weights[13]};
}

// `stale`: bit g = group g's image is rebuilt by this call (the host's dirty flag); the blocks of any other group have nothing to do
__global__ __launch_bounds__(256) void iqn_group_consts_kernel(const IqnActorRow *__restrict__ table, uint64_t stale) {
    if (!((stale >> blockIdx.y) & 1ull)) return;
    const IqnActorRow &r = table[blockIdx.y];
    split_consts_block(actor_weights(r), r.consts);
}

// iqn_split_prep_kernel per group: blocks [0, pack_blocks) pack a stale group's image (pack_blocks = 0 when no group is stale), the others draw
__global__ __launch_bounds__(256) void iqn_group_prep_kernel(const IqnActorRow *__restrict__ table, uint64_t stale, int n, float cvar, int pack_blocks,
                                                             float eps, int32_t *__restrict__ actions_all, int listed) {
    const IqnActorRow &r = table[blockIdx.y];
    if ((int)blockIdx.x < pack_blocks) {
        if (!((stale >> blockIdx.y) & 1ull)) return;
        const int i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i < OFF_FB) r.packed[i] = pack_word(actor_weights(r), r.consts, i);
        return;
    }
    if (listed) draw_block<true>(r.rng_state, r.draws, n, nullptr, cvar, pack_blocks, eps, actions_all + (size_t)blockIdx.y * n,
                                 GreedyRows{reinterpret_cast<int32_t *>(r.rows_buf + 4), r.rows_buf});
    else draw_block(r.rng_state, r.draws, n, nullptr, cvar, pack_blocks);
}

// the acting forms <QUANT = false, SHARED = false, WAVES, LATE = false, ROWS> of iqn_qvals_split_kernel on grid (workgroups per group, G)
template <bool ROWS>
__global__ __launch_bounds__(64 * WAVES) void iqn_group_act_kernel(const IqnActorRow *__restrict__ table, const float *__restrict__ obs_all, float eps,
                                                                   int32_t *__restrict__ actions_all, int n) {
    constexpr bool QUANT = false, SHARED = false, LATE = false;
    constexpr int NW = WAVES;
    const IqnActorRow &r = table[blockIdx.y];
    const float *__restrict__ obs = obs_all + (size_t)blockIdx.y * n * OBS;
    const float *__restrict__ taus = r.draws;
    const uint32_t *__restrict__ packed = r.packed;
    float *__restrict__ qvals = nullptr;
    const float *__restrict__ explore_u = eps > 0.f ? r.draws + (size_t)n * K_TAUS : nullptr;
    int32_t *__restrict__ actions = actions_all + (size_t)blockIdx.y * n;
    uint64_t *__restrict__ rng_state = r.rng_state;
    float *__restrict__ quantiles = nullptr;
    [[maybe_unused]] const float *__restrict__ h1 = nullptr;
    [[maybe_unused]] LateRows late = {};      // (no late rows in the grouped forms)
    [[maybe_unused]] const GreedyRows rows = {reinterpret_cast<int32_t *>(r.rows_buf + 4), r.rows_buf};
#include "iqn_act_split_body.h"
}

}  // namespace sp
