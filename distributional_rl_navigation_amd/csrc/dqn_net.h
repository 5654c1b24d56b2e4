// dqn_net.h -- the DQN baseline's network on the matrix pipe, shared by dqn_act.hip (one act launch) and mn_rollout_dqn.hip (whole episodes in one
// launch).  Included INSIDE the including file's anonymous namespace.  Layout and k order are documented at the top of dqn_act.hip; both kernels run
// the same seven dense<> stages on the same LDS image, so an environment gets the same bits from either, whichever MFMA column it sits in (a column
// of the C tile depends on its own column of B only).
#pragma once

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int OBS = MN_OBS_DIM;      // 26
constexpr int F = 208, H = 64, A = 9;
// stages: the encoders (one block-diagonal matrix) + hidden_layer + hidden_layer_2 + output_layer + q_net.0 + q_net.2 + q_net.4, each as
// (M tiles of 16 outputs, K tiles of 16 inputs).  LDS image (floats): per stage [mt][kt][64 lanes][4 r] weights, then the biases padded
// to multiples of 16
constexpr int N_LAYERS = 7;
constexpr int LM[N_LAYERS] = {13, 4, 4, 1, 4, 4, 1}, LK[N_LAYERS] = {2, 13, 4, 4, 1, 4, 4};
constexpr int lw_off(int l) { int o = 0; for (int i = 0; i < l; ++i) o += LM[i] * LK[i] * 256; return o; }
constexpr int OFF_BIAS = lw_off(N_LAYERS);
constexpr int lb_off(int l) { int o = OFF_BIAS; for (int i = 0; i < l; ++i) o += LM[i] * 16; return o; }
constexpr int IMAGE_FLOATS = lb_off(N_LAYERS);
static_assert(IMAGE_FLOATS * 4 <= 160 * 1024, "the DQN weight image must fit the CU's LDS");
static_assert(IMAGE_FLOATS % 4 == 0, "16-byte copy");

// out[mt] = act(W_l in + b_l) for one 16-env tile: in[t][r] = input feature 16 t + 4 g + r of env col
template <int L, bool RELU, int MT, int KT>
__device__ __forceinline__ void dense(const float *__restrict__ lds, int lane, const f32x4 (&in)[KT], f32x4 (&out)[MT]) {
    const f32x4 *w4 = reinterpret_cast<const f32x4 *>(lds + lw_off(L)) + lane;
    const f32x4 *b4 = reinterpret_cast<const f32x4 *>(lds + lb_off(L)) + (lane >> 4);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        f32x4 acc = b4[4 * mt];      // bias[16 mt + 4 g + r]: the accumulator's initial value
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const f32x4 a = w4[(mt * KT + t) * 64];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], in[t][r], acc, 0, 0, 0);
        }
        if (RELU) { acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f); }
        out[mt] = acc;
    }
}

// Q(s, .) of the 16 envs of a tile: x0[t][r] = observation feature 16 t + 4 g + r of env col (26 inputs, zero-padded to 32); lane (g, col) gets
// the Q-values of actions 4 g + r of env col (rows 9..15 are zero)
__device__ __forceinline__ f32x4 dqn_forward(const float *__restrict__ lds, int lane, const f32x4 (&x0)[2]) {
    f32x4 f[13], h1[4], h2[4], o[1], q1[4], q2[4], q[1];
    dense<0, false, 13, 2>(lds, lane, x0, f);        // the three encoders, no activation (torch_layers.py:125-128)
    dense<1, true, 4, 13>(lds, lane, f, h1);         // hidden_layer + ReLU
    dense<2, true, 4, 4>(lds, lane, h1, h2);         // hidden_layer_2 + ReLU
    dense<3, false, 1, 4>(lds, lane, h2, o);         // output_layer: the extractor's 9 "features" (rows 9..15 are zero)
    dense<4, true, 4, 1>(lds, lane, o, q1);          // q_net.0 + ReLU
    dense<5, true, 4, 4>(lds, lane, q1, q2);         // q_net.2 + ReLU
    dense<6, false, 1, 4>(lds, lane, q2, q);         // q_net.4: Q(s, a), lane (g, col) holds actions 4 g + r of env col
    return q[0];
}

// first maximum over the 9 actions of env col: in-lane over r, then across the four lane groups; every lane of the column gets the result
__device__ __forceinline__ int dqn_argmax(const f32x4 &q, int g) {
    float best = -INFINITY;
    int arg = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int a_idx = 4 * g + r;
        const float v = a_idx < A ? q[r] : -INFINITY;
        if (v > best) { best = v; arg = a_idx; }
    }
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
        const float ob = __shfl_xor(best, off);
        const int oa = __shfl_xor(arg, off);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    return arg;
}
