// iqn_act_common.h -- what the IQN act kernels (iqn_act_exact.h, iqn_act_split.h, iqn_act_tiled.h) and the IQN episode rollout share: the network's
// widths, the weight pointers, the tau-row sum and the counter-based draws of an act call.  Included by iqn_act.hip and mn_rollout_iqn.hip inside
// their anonymous namespaces, in front of the kernel headers.

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int K_TAUS = 32;      // model.py:118
constexpr int N_COS = 64;       // model.py:130
constexpr int F = 208;          // 16 + 16 + 176 feature width
constexpr int H = 64;           // hidden width
constexpr int A_OUT = 9;        // actions
constexpr int T1 = F / 16;      // 13 feature tiles
constexpr int OBS = MN_OBS_DIM;                   // 26
constexpr int OBS4 = 7;                           // 26 inputs padded to 7 float4

// sum over the 16 lanes of a row (lanes sharing l >> 4)
__device__ __forceinline__ float row_sum16(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad xor 1
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // quad xor 2
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));  // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));  // row_mirror
    return v;
}

struct IqnWeights {   // device pointers, nn.Linear layout [out][in]
    const float *ve_w, *ve_b, *ge_w, *ge_b, *se_w, *se_b;   // velocity / goal / sensor encoders
    const float *W1, *b1, *W2, *b2, *W3, *b3, *W4, *b4;     // cos_embedding, hidden_layer, hidden_layer_2, output_layer
};

// Counter-based uniform draws: draw number `idx` of call `ctr` is a double murmur3-fmix32 of the index under two 32-bit
// keys derived from (seed, ctr) -- no generator state per element, any element can be produced by any thread.
__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ float u01(uint32_t idx, uint32_t k0, uint32_t k1) {      // 24-bit uniform in [0, 1), like torch.rand
    return (float)(fmix32(fmix32(idx ^ k0) + k1) >> 8) * (1.0f / 16777216.0f);
}
// the two keys of act call number `ctr` under `seed` (rng_state = {seed, ctr})
__device__ __forceinline__ void draw_keys(uint64_t seed, uint64_t ctr, uint32_t &k0, uint32_t &k1) {
    const uint64_t base = mix64(seed + 0x9E3779B97F4A7C15ull * (ctr + 1));
    k0 = (uint32_t)base; k1 = (uint32_t)(base >> 32);
}
// tau j of row e of an act call with per-environment taus: U[0,1) x the row's cvar (model.py:149-153)
__device__ __forceinline__ float tau_draw(int e, int j, uint32_t k0, uint32_t k1, float cvar) {
    return u01((uint32_t)((long)e * K_TAUS + j), k0, k1) * cvar;
}

// IQNAgent.act's random action of an exploring row (agent.py:199-203, !(u > eps)): one function for every kernel that writes it, so the bits cannot differ
__device__ __forceinline__ int explore_action(float u, float eps) {
    const int act = (int)(u / eps * (float)A_OUT);
    return act > A_OUT - 1 ? A_OUT - 1 : act;
}

// The rows of an act call that need the network (mn_iqn_set_greedy_rows): the preparation launch, which draws every row's exploration uniform, writes the
// action of an exploring row itself and appends every other row to `list` (any order); the act kernel then deals the list out evenly.  words[0], [1] = two
// count slots used in turn, [2] = the slot of the call in flight (preparation -> act kernel), [3] = the slot of the next call (act kernel -> preparation):
// the preparation launch zeroes the slot it does not count in, so the count is re-armed on the device, without a launch or a memset of its own.
struct GreedyRows {
    int32_t *list;        // [n]
    uint32_t *words;      // [4]
};

// The random numbers of one act call: blocks [pack_blocks, gridDim.x) fill draws[0 .. 32 n) with tau = U[0,1) * cvar
// (model.py:149-153; per-row cvar if cvar_row) and draws[32 n .. 33 n) with the exploration uniforms of IQNAgent.act
// (agent.py:199).  ROWS: the thread that draws row e's uniform also settles the row -- actions[e] for an exploring row, an entry of rows.list for any
// other; a wavefront's entries are counted by ballot and appended with one atomic.  BT = threads of a drawing block (the draws are counter-based: what
// is drawn does not depend on it; 64 in the launch that also resets episodes, mn_prep_reset.hip); `pack_blocks` = the launch's blocks in front of them.
template <bool ROWS = false, int BT = 256>
__device__ __forceinline__ void draw_block(const uint64_t *__restrict__ rng_state, float *__restrict__ draws, int n,
                                           const float *__restrict__ cvar_row, float cvar, int pack_blocks, float eps = 0.f,
                                           int32_t *__restrict__ actions = nullptr, const GreedyRows rows = {}) {
    uint32_t k0, k1;
    draw_keys(rng_state[0], rng_state[1], k0, k1);
    [[maybe_unused]] uint32_t slot = 0;
    if constexpr (ROWS) {
        slot = rows.words[3] & 1u;
        if ((int)blockIdx.x == pack_blocks && threadIdx.x == 0) { rows.words[slot ^ 1u] = 0u; rows.words[2] = slot; }
    }
    const long total4 = ((long)n * (K_TAUS + 1) + 3) / 4;          // float4 groups
    const long stride = (long)((int)gridDim.x - pack_blocks) * BT;
    for (long q = (long)((int)blockIdx.x - pack_blocks) * BT + threadIdx.x; q < total4; q += stride) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long idx = 4 * q + j;
            float u = u01((uint32_t)idx, k0, k1);
            if (idx < (long)n * K_TAUS) u *= cvar_row ? cvar_row[idx / K_TAUS] : cvar;
            v[j] = u;
        }
        if (4 * q + 3 < (long)n * (K_TAUS + 1)) *reinterpret_cast<float4 *>(draws + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
        else
            for (int j = 0; j < 4 && 4 * q + j < (long)n * (K_TAUS + 1); ++j) draws[4 * q + j] = v[j];
        if constexpr (ROWS) {      // (the lanes of a wavefront leave this loop from the top lane down: ballots count the lanes still in it)
            const int lane = threadIdx.x & 63;
            const long e0 = 4 * q - (long)n * K_TAUS;      // row of v[0]
            bool keep[4];
            int at[4], total = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool row = e0 + j >= 0 && e0 + j < n;
                keep[j] = row && v[j] > eps;               // greedy iff u > eps (agent.py:200)
                if (row && !keep[j]) actions[e0 + j] = explore_action(v[j], eps);
                const unsigned long long m = __ballot(keep[j]);
                at[j] = total + __popcll(m & ((1ull << lane) - 1ull));
                total += __popcll(m);
            }
            if (total) {
                const int leader = __builtin_ctzll(__ballot(true));
                int base = 0;
                if (lane == leader) base = (int)atomicAdd(rows.words + slot, (uint32_t)total);
                base = __shfl(base, leader);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (keep[j] && base + at[j] < n) rows.list[base + at[j]] = (int32_t)(e0 + j);      // (< n: always, while the slot started at zero)
            }
        }
    }
}
