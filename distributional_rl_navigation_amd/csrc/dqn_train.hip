// dqn_train.hip -- fused gradient step of the DQN baseline for gfx950 (MI355X): batch draw, target and local forward, smooth-L1
// TD loss, backward, gradient-norm clip and Adam in ONE launch.
//
// Replaces, for one optimizer step of DQNAgent.train (the reference's stable-baselines3 `DQN.train`, dqn/dqn.py:188-230) on a batch
// drawn from the device replay ring:
//     next_q   = q_net_target(next_obs).max(dim = 1)                      (:198-201)
//     target_q = r + (1 - done) * gamma * next_q                          (:203)
//     current  = q_net(obs).gather(1, a)                                  (:206-209)
//     loss     = smooth_l1_loss(current, target_q)      (beta 1, mean)    (:212)
//     backward; clip_grad_norm_(10); Adam(lr 1e-4)                        (:216-221)
// with the network of dqn_act.hip (26 -> (16 | 16 | 176) encoders without activation, 208 -> 64 -> 64 -> 9, then 9 -> 64 -> 64 -> 9,
// ReLU after hidden_layer, hidden_layer_2, q_net.0 and q_net.2).  27 650 parameters, ~28 k multiply-adds per sample and pass.
//
// Decomposition: ceil(B / 16) workgroups of 512 threads.  Workgroup w owns batch slots [16 w, 16 w + 16) -- one MFMA tile of samples --
// and carries it through the target forward, the local forward, the loss and the whole backward with its activations in LDS.  It writes
// its partial parameter gradient (every element exactly once) into row w of the workspace and its partial loss next to it, publishes them
// (agent-scope release) and takes a ticket.  The workgroup that takes the LAST ticket (agent-scope acquire) sums the rows in index order,
// forms the global norm, clips, applies Adam over the flat vectors and advances the step and call counters.  No float atomics, no waits,
// no co-residency: the result does not depend on which workgroup finishes last.
//
// MFMA mapping: exact-f32 v_mfma_f32_16x16x4_f32.  Every product is a 16 x 16 tile C[i][j] = sum_k A(i, k) B(k, j), lane (l, g) =
// (lane & 15, lane >> 4) feeding A(l, k0 + g) and B(k0 + g, l), and holding C[4 g + r][l] afterwards.  Forward tiles are [16 samples x
// 16 outputs] (A = activations in LDS, B = the layer's weights read straight from the flat parameter vector: they change every step),
// data-gradient tiles [16 samples x 16 inputs], weight-gradient tiles [16 outputs x 16 inputs] contracted over the 16 samples.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <new>

#include "marinenav_hip.h"
#include "mn_train_shared.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int OBS = MN_OBS_DIM;      // 26
constexpr int F = 208, H = 64, A = 9;
constexpr int THREADS = 512, WAVES = THREADS / 64, TILE = 16, MAX_BATCH_DQN = 256;
// flat parameter vector = DQNPolicy.q_net.named_parameters() order, nn.Linear [out][in]
constexpr int O_VW = 0, O_VB = 32, O_GW = 48, O_GB = 80, O_SW = 96, O_SB = 3968, O_HW = 4144, O_HB = 17456, O_H2W = 17520, O_H2B = 21616,
              O_OW = 21680, O_OB = 22256, O_Q0W = 22265, O_Q0B = 22841, O_Q2W = 22905, O_Q2B = 27001, O_Q4W = 27065, O_Q4B = 27641,
              P_TOTAL = 27650;
static_assert(O_Q4B + A == P_TOTAL, "flat parameter layout");
constexpr int P_PAD = 27652;         // row stride of the partial gradients (16-byte aligned rows)
// workspace (floats): [n_part][P_PAD] partial gradients | [16] partial losses | ticket (u32) + padding
__host__ __device__ constexpr int64_t ws_loss(int n_part) { return (int64_t)n_part * P_PAD; }
__host__ __device__ constexpr int64_t ws_ticket(int n_part) { return ws_loss(n_part) + 16; }
__host__ __device__ constexpr int64_t ws_total(int n_part) { return ws_ticket(n_part) + 4; }

// LDS (floats): row strides of the [16 samples][width] activation blocks
constexpr int LDO = 28, LDF = 212, LDH = 68, LDA = 16, LDD = 212;
constexpr int S_OBS = 0;                        // [16][LDO] states
constexpr int S_NOBS = S_OBS + TILE * LDO;      // [16][LDO] next_states
constexpr int S_F = S_NOBS + TILE * LDO;        // [16][LDF] encoder outputs
constexpr int S_H1 = S_F + TILE * LDF;          // [16][LDH] relu(hidden_layer)
constexpr int S_H2 = S_H1 + TILE * LDH;         // [16][LDH] relu(hidden_layer_2)
constexpr int S_O = S_H2 + TILE * LDH;          // [16][LDA] output_layer (the extractor's 9 features)
constexpr int S_Q1 = S_O + TILE * LDA;          // [16][LDH] relu(q_net.0)
constexpr int S_Q2 = S_Q1 + TILE * LDH;         // [16][LDH] relu(q_net.2)
constexpr int S_Q = S_Q2 + TILE * LDH;          // [16][LDA] Q values
constexpr int S_D0 = S_Q + TILE * LDA;          // [16][LDD] gradient ping-pong buffers
constexpr int S_D1 = S_D0 + TILE * LDD;
constexpr int S_Y = S_D1 + TILE * LDD;          // [16] TD targets
constexpr int S_TOTAL = S_Y + TILE;
static_assert(S_TOTAL * 4 <= 64 * 1024, "static LDS");

// A tile of 16 samples is carried by a GROUP of 512 threads (8 waves).  The single step's workgroup is one group; the chain of the multi-step call
// (below) holds one group per tile.  The layer templates take the thread index `tid` as an argument and address a thread by its place in its group, so
// both run the same instructions per element -- and a kernel that LOOPS over steps can hand them an index the compiler cannot see through, which keeps
// it from hoisting every per-lane address of every layer in front of the loop (hundreds of registers: the loop kernels spilled to scratch).
__device__ __forceinline__ int lane_of(int tid) { return tid & 63; }
__device__ __forceinline__ int ltid_of(int tid) { return tid & (THREADS - 1); }
__device__ __forceinline__ int wave_of(int tid) { return ltid_of(tid) >> 6; }

// acc[i][j] += sum_{k < K} A(i, k) B(k, j) on one 16 x 16 tile; lane (l, g) reads A(l, k) and B(k, l) for k = k0 + g
template <int K, class FA, class FB>
__device__ __forceinline__ f32x4 mma16(FA fa, FB fb, f32x4 acc, int tid) {
    const int l = lane_of(tid) & 15, g = lane_of(tid) >> 4;
#pragma unroll
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + g;
        const float a = k < K ? fa(l, k) : 0.f;
        const float b = k < K ? fb(k, l) : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
    return acc;
}

// forward, output tile nt of a layer with weights W [N][K], bias b: Y[s][n] = act(X[s][:K] . W[n] + b[n]); columns N.. of the last tile get 0
template <int K, int N, bool RELU>
__device__ __forceinline__ void fwd_tile(const float *X, int ldx, const float *__restrict__ W, const float *__restrict__ b, int nt, float *Y, int ldy, int tid) {
    const int l = lane_of(tid) & 15, g = lane_of(tid) >> 4, n = 16 * nt + l;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = mma16<K>([&](int i, int k) { return X[i * ldx + k]; }, [&](int k, int) { return n < N ? W[n * K + k] : 0.f; }, acc, tid);
    const float bn = n < N ? b[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float y = acc[r] + bn;
        if (RELU) y = fmaxf(y, 0.f);
        Y[(4 * g + r) * ldy + n] = n < N ? y : 0.f;
    }
}

// the whole network on the 16 samples in `obs` (LDS) with the flat parameters P; activations stay in LDS
__device__ __forceinline__ void forward(const float *__restrict__ P, const float *obs, float *S, int tid) {
    const int wave = wave_of(tid);
    for (int t = wave; t < 13; t += WAVES) {      // the three encoders, no activation: 1 + 1 + 11 output tiles
        if (t == 0) fwd_tile<2, 16, false>(obs, LDO, P + O_VW, P + O_VB, 0, S + S_F, LDF, tid);
        else if (t == 1) fwd_tile<2, 16, false>(obs + 2, LDO, P + O_GW, P + O_GB, 0, S + S_F + 16, LDF, tid);
        else fwd_tile<22, 176, false>(obs + 4, LDO, P + O_SW, P + O_SB, t - 2, S + S_F + 32, LDF, tid);
    }
    __syncthreads();
    if (wave < 4) fwd_tile<F, H, true>(S + S_F, LDF, P + O_HW, P + O_HB, wave, S + S_H1, LDH, tid);      // hidden_layer + ReLU
    __syncthreads();
    if (wave < 4) fwd_tile<H, H, true>(S + S_H1, LDH, P + O_H2W, P + O_H2B, wave, S + S_H2, LDH, tid);   // hidden_layer_2 + ReLU
    __syncthreads();
    if (wave == 0) fwd_tile<H, A, false>(S + S_H2, LDH, P + O_OW, P + O_OB, 0, S + S_O, LDA, tid);       // output_layer
    __syncthreads();
    if (wave < 4) fwd_tile<A, H, true>(S + S_O, LDA, P + O_Q0W, P + O_Q0B, wave, S + S_Q1, LDH, tid);    // q_net.0 + ReLU
    __syncthreads();
    if (wave < 4) fwd_tile<H, H, true>(S + S_Q1, LDH, P + O_Q2W, P + O_Q2B, wave, S + S_Q2, LDH, tid);   // q_net.2 + ReLU
    __syncthreads();
    if (wave == 0) fwd_tile<H, A, false>(S + S_Q2, LDH, P + O_Q4W, P + O_Q4B, 0, S + S_Q, LDA, tid);     // q_net.4: Q(s, .)
    __syncthreads();
}

// backward through one layer Y = X W^T + b with dY [16][N] (row stride LDD) in LDS:
//   gb[o] = sum_s dY[s][o]; gW[o][k] = sum_s dY[s][o] X[s][k] (tiles [16 o x 16 k] over the 16 samples);
//   if DX: dX[s][k] = sum_o dY[s][o] W[o][k], times [X[s][k] > 0] when X is a ReLU output (MASK)
template <int K, int N, bool DX, bool MASK>
__device__ __forceinline__ void bwd_layer(const float *dY, const float *X, int ldx, const float *__restrict__ W, float *gW, float *gb, float *dX, int tid) {
    constexpr int MT = (N + 15) / 16, KT = (K + 15) / 16, NT = MT * KT + (DX ? KT : 0);
    const int l = lane_of(tid) & 15, g = lane_of(tid) >> 4;
    if (ltid_of(tid) < N) {
        float s = 0.f;
        for (int i = 0; i < TILE; ++i) s += dY[i * LDD + ltid_of(tid)];
        gb[ltid_of(tid)] = s;
    }
    for (int t = wave_of(tid); t < NT; t += WAVES) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (t < MT * KT) {
            const int mo = t / KT, k = 16 * (t % KT) + l;
            acc = mma16<TILE>([&](int i, int s) { return dY[s * LDD + 16 * mo + i]; }, [&](int s, int) { return k < K ? X[s * ldx + k] : 0.f; }, acc, tid);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = 16 * mo + 4 * g + r;
                if (o < N && k < K) gW[o * K + k] = acc[r];
            }
        } else {
            const int k = 16 * (t - MT * KT) + l;
            acc = mma16<N>([&](int i, int o) { return dY[i * LDD + o]; }, [&](int o, int) { return k < K ? W[o * K + k] : 0.f; }, acc, tid);
            if (k < K)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = 4 * g + r;
                    dX[s * LDD + k] = (!MASK || X[s * ldx + k] > 0.f) ? acc[r] : 0.f;
                }
        }
    }
}

__device__ __forceinline__ float sumsq4(float a, float b, float c, float d) { return fmaf(d, d, fmaf(c, c, fmaf(b, b, a * a))); }

struct DqnTrainArgs {
    const float *states, *next_states;
    const int64_t *actions;
    const float *rewards, *dones;
    int64_t ring_size;
    uint64_t *rng_state;         // {seed, call counter} or NULL
    const int64_t *idx;          // given rows (rng_state == NULL)
    int64_t *idx_out;            // or NULL
    float *params;
    const float *target;
    float *ws, *grad, *loss, *m, *v;
    int32_t *step;
    int batch;
    float gamma;
    double lr, b1, b2, eps, max_norm;
};

// One workgroup of one learner's step: workgroup blockIdx.x of gridDim.x.  The body of dqn_train_step_kernel AND of dqn_train_step_groups_kernel (below,
// where blockIdx.y picks the learner whose buffers `a` names): one instruction sequence per output element, whichever kernel it is inlined into.
__device__ __forceinline__ void dqn_train_step_body(const DqnTrainArgs &a) {
    __shared__ __attribute__((aligned(16))) float S[S_TOTAL];      // (the LDS of whichever kernel inlines the body)
    __shared__ int s_act[TILE];
    __shared__ float s_red[WAVES];
    __shared__ float s_misc[4];      // loss terms' sum, clip coefficient, Adam step size, sqrt of the second bias correction
    __shared__ int s_last;
    const int tid = threadIdx.x, n_part = gridDim.x;
    const int slot0 = blockIdx.x * TILE;
    float *part = a.ws + (int64_t)blockIdx.x * P_PAD;

    // ---- this workgroup's 16 transitions (slots past the batch: zero observations, no gradient)
    const uint64_t base = a.rng_state ? sample_base(a.rng_state) : 0;
    if (tid < TILE * LDO) {
        const int s = tid / LDO, c = tid % LDO, b = slot0 + s;
        const bool live = b < a.batch;
        int64_t row = 0;
        if (live) row = a.rng_state ? (int64_t)perm_row(base, (uint32_t)a.ring_size, (uint32_t)b) : a.idx[b];
        const bool in = live && c < OBS;
        S[S_OBS + s * LDO + c] = in ? a.states[row * OBS + c] : 0.f;
        S[S_NOBS + s * LDO + c] = in ? a.next_states[row * OBS + c] : 0.f;
        if (c == 0) {
            int64_t act = live ? a.actions[row] : 0;
            s_act[s] = (act >= 0 && act < A) ? (int)act : 0;
            if (live && a.idx_out) a.idx_out[b] = row;
            S[S_Y + s] = 0.f;
            if (live) {      // park r and done in the gradient buffer until the target forward has run
                S[S_D0 + s] = a.rewards[row];
                S[S_D0 + TILE + s] = a.dones[row];
            }
        }
    }
    __syncthreads();
    float rew = 0.f, done = 0.f;
    if (tid < TILE && slot0 + tid < a.batch) { rew = S[S_D0 + tid]; done = S[S_D0 + TILE + tid]; }

    // ---- TD target: r + (1 - done) gamma max_a Q_target(s', a)
    forward(a.target, S + S_NOBS, S, tid);
    if (tid < TILE && slot0 + tid < a.batch) {
        float mx = S[S_Q + tid * LDA];
        for (int j = 1; j < A; ++j) mx = fmaxf(mx, S[S_Q + tid * LDA + j]);
        const float t = (1.f - done) * a.gamma;
        S[S_Y + tid] = rew + t * mx;
    }
    // ---- local forward (the barrier at its head orders the TD targets), loss, dL/dQ
    forward(a.params, S + S_OBS, S, tid);
    if (tid < TILE) {
        const bool live = slot0 + tid < a.batch;
        const float d = S[S_Q + tid * LDA + s_act[tid]] - S[S_Y + tid];
        const float ad = fabsf(d);
        const float term = ad < 1.f ? 0.5f * d * d : ad - 0.5f;       // smooth_l1, beta = 1
        const float gq = (ad < 1.f ? d : copysignf(1.f, d)) * (1.f / (float)a.batch);
        for (int j = 0; j < LDA; ++j) S[S_D0 + tid * LDD + j] = (live && j == s_act[tid]) ? gq : 0.f;
        S[S_Y + tid] = live ? term : 0.f;
    }
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int s = 0; s < TILE; ++s) t += S[S_Y + s];
        a.ws[ws_loss(n_part) + blockIdx.x] = t;
    }

    // ---- backward, output layer first; D0 / D1 alternate as dY and dX
    bwd_layer<H, A, true, true>(S + S_D0, S + S_Q2, LDH, a.params + O_Q4W, part + O_Q4W, part + O_Q4B, S + S_D1, tid);      // q_net.4
    __syncthreads();
    bwd_layer<H, H, true, true>(S + S_D1, S + S_Q1, LDH, a.params + O_Q2W, part + O_Q2W, part + O_Q2B, S + S_D0, tid);      // q_net.2
    __syncthreads();
    bwd_layer<A, H, true, false>(S + S_D0, S + S_O, LDA, a.params + O_Q0W, part + O_Q0W, part + O_Q0B, S + S_D1, tid);      // q_net.0
    __syncthreads();
    bwd_layer<H, A, true, true>(S + S_D1, S + S_H2, LDH, a.params + O_OW, part + O_OW, part + O_OB, S + S_D0, tid);         // output_layer
    __syncthreads();
    bwd_layer<H, H, true, true>(S + S_D0, S + S_H1, LDH, a.params + O_H2W, part + O_H2W, part + O_H2B, S + S_D1, tid);      // hidden_layer_2
    __syncthreads();
    bwd_layer<F, H, true, false>(S + S_D1, S + S_F, LDF, a.params + O_HW, part + O_HW, part + O_HB, S + S_D0, tid);         // hidden_layer
    __syncthreads();
    bwd_layer<2, 16, false, false>(S + S_D0, S + S_OBS, LDO, nullptr, part + O_VW, part + O_VB, nullptr, tid);               // encoders
    bwd_layer<2, 16, false, false>(S + S_D0 + 16, S + S_OBS + 2, LDO, nullptr, part + O_GW, part + O_GB, nullptr, tid);
    bwd_layer<22, 176, false, false>(S + S_D0 + 32, S + S_OBS + 4, LDO, nullptr, part + O_SW, part + O_SB, nullptr, tid);

    // ---- publish the row (agent-scope release before the ticket), the last arriver acquires and finishes the step
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        unsigned *ticket = reinterpret_cast<unsigned *>(a.ws + ws_ticket(n_part));
        const unsigned old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old == (unsigned)n_part - 1u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;

    // ---- last workgroup: gradient = sum of the rows in index order, its squared norm in a fixed order
    float sq = 0.f;
    for (int q = tid; q < P_PAD / 4; q += THREADS) {
        float4 g = reinterpret_cast<const float4 *>(a.ws)[q];
        for (int w = 1; w < n_part; ++w) {
            const float4 x = reinterpret_cast<const float4 *>(a.ws + (int64_t)w * P_PAD)[q];
            g.x += x.x; g.y += x.y; g.z += x.z; g.w += x.w;
        }
        const float e[4] = {g.x, g.y, g.z, g.w};
        float e2[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int p = 4 * q + c;
            e2[c] = p < P_TOTAL ? e[c] : 0.f;
            if (p < P_TOTAL) a.grad[p] = e[c];
        }
        sq += sumsq4(e2[0], e2[1], e2[2], e2[3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
    if (lane_of(tid) == 0) s_red[wave_of(tid)] = sq;
    __syncthreads();
    if (tid == 0) {
        float tot = 0.f;
        for (int w = 0; w < WAVES; ++w) tot += s_red[w];
        const float norm = sqrtf(tot);
        s_misc[1] = fminf((float)a.max_norm / (norm + 1e-6f), 1.f);      // clip_grad_norm_: coef = max_norm / (norm + 1e-6), clamped to 1
        float l = 0.f;
        for (int w = 0; w < n_part; ++w) l += a.ws[ws_loss(n_part) + w];
        a.loss[0] = l / (float)a.batch;
        const int t_step = *a.step + 1;
        // python-float (double) scalars of torch's Adam, rounded to float32 where the tensor kernels consume them (as iqn_adam)
        s_misc[2] = (float)(a.lr / (1.0 - pow(a.b1, (double)t_step)));
        s_misc[3] = (float)sqrt(1.0 - pow(a.b2, (double)t_step));
        *a.step = t_step;
        if (a.rng_state) a.rng_state[1] = a.rng_state[1] + 1;
    }
    __syncthreads();
    const float coef = s_misc[1], step_size = s_misc[2], bc2_sqrt = s_misc[3];
    const float w1 = (float)(1.0 - a.b1), b2f = (float)a.b2, w2 = (float)(1.0 - a.b2), eps = (float)a.eps;
    // ---- clip + Adam, same element mapping as the sum above (each thread re-reads its own gradient stores)
    for (int q = tid; q < P_PAD / 4; q += THREADS)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int p = 4 * q + c;
            if (p >= P_TOTAL) continue;
            const float gq = a.grad[p] * coef;
            a.grad[p] = gq;
            float mm = a.m[p], vv = a.v[p], pp = a.params[p];
            adam_update(gq, mm, vv, pp, w1, b2f, w2, step_size, bc2_sqrt, eps);
            a.m[p] = mm;
            a.v[p] = vv;
            a.params[p] = pp;
        }
}

__global__ __launch_bounds__(THREADS) void dqn_train_step_kernel(const DqnTrainArgs a) {
    dqn_train_step_body(a);
}


// ---- many steps per call (mn_dqn_train_steps) ----------------------------------------------------------------------------------------------------------
// n_steps consecutive steps of the kernel above from one call, bit for bit: the same tiles, the same instruction sequence per output element and the
// same summation orders.  Two facts a single launch cannot use:
//   * the TD targets of ALL steps are known up front -- the target network and the ring are constant while the steps run and the rows of step k depend
//     only on {seed, call counter + k, ring_size} -- so one device-wide launch (dqn_multi_target_kernel) computes y[k][b] for every sample;
//   * at batch <= 32 the remaining chain -- local forward, loss, backward, ordered sum, clip, Adam -- fits ONE workgroup: one 512-thread group per tile,
//     each with its own activations in LDS (2 x 63.8 KB of the CU's 160 KiB), looping over the steps (dqn_multi_chain_kernel).  No ticket, no launch
//     boundary between steps, no workgroup that waits on another.
// What one step stores and the next (or the next phase) loads -- the partial gradient rows, the gradient, the moments and the parameters -- goes through
// memory and is re-read through the same CU's vector L1: behind every such hand-off the workgroup waits for its stores, meets at a barrier and
// invalidates the L1 (agent-scope acquire), or the loads could be served lines from before the stores.
constexpr int MAX_STEPS = MN_DQN_MAX_STEPS, CHAIN_TILES = 2, CHAIN_THREADS = CHAIN_TILES * THREADS, CHAIN_BATCH = CHAIN_TILES * TILE;
static_assert(CHAIN_TILES * S_TOTAL * 4 + 1024 <= 160 * 1024, "the chain's activations fit the LDS of one gfx950 CU");
// workspace (floats): [2][P_PAD] partial gradients | [n_steps][32] TD targets, y[k * batch + b] | [n_steps][2] Adam step size and sqrt of the second bias correction
__host__ __device__ constexpr int64_t ms_y() { return (int64_t)CHAIN_TILES * P_PAD; }
__host__ __device__ constexpr int64_t ms_adam(int n_steps) { return ms_y() + (int64_t)n_steps * CHAIN_BATCH; }
__host__ __device__ constexpr int64_t ms_total(int n_steps) { return ms_adam(n_steps) + 2 * (int64_t)n_steps + 4; }

struct DqnStepsArgs : DqnTrainArgs {      // loss: [n_steps]; idx / idx_out: [n_steps][batch]
    int n_steps;
    // float32 constants of every step, rounded on the host exactly as the single step rounds them on the device (IEEE conversions and one division): as
    // kernel arguments they sit in scalar registers, where the step loop can carry them for nothing
    float w1, b2f, w2, eps_f, batch_f, inv_batch;
};

// The thread index as a value the compiler cannot trace to threadIdx.x: asked for once per iteration of a step loop, it keeps what derives from it inside.
__device__ __forceinline__ int opaque(int tid) {
    asm volatile("" : "+v"(tid));
    return tid;
}

// __shfl_xor on the opaque thread index
__device__ __forceinline__ float shfl_xor_of(float v, int off, int tid) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(((tid ^ off) & 63) << 2, __float_as_int(v)));
}

// Stores -> barrier -> L1 invalidate: what the workgroup wrote before is what it loads after.
__device__ __forceinline__ void chain_handoff() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// TD targets of all n_steps x batch samples, 16 consecutive samples (k, b) = (j / batch, j % batch) per tile -- a sample's Q row depends on its own MFMA row
// only, so the regrouping does not change a bit -- and the double-precision Adam scalars of every step, off the chain.
// (The body of dqn_multi_target_kernel and of its grouped form: tiles over blockIdx.x of gridDim.x.)
__device__ __forceinline__ void dqn_multi_target_body(const DqnStepsArgs &a) {
    __shared__ __attribute__((aligned(16))) float S[S_TOTAL];
    const int total = a.n_steps * a.batch;
    const uint64_t seed = a.rng_state ? a.rng_state[0] : 0, counter = a.rng_state ? a.rng_state[1] : 0;
    float *y = a.ws + ms_y(), *adam = a.ws + ms_adam(a.n_steps);
    const int step0 = *a.step;
    for (int k = blockIdx.x * THREADS + (int)threadIdx.x; k < a.n_steps; k += gridDim.x * THREADS) {
        const int t_step = step0 + k + 1;
        adam[2 * k] = (float)(a.lr / (1.0 - pow(a.b1, (double)t_step)));
        adam[2 * k + 1] = (float)sqrt(1.0 - pow(a.b2, (double)t_step));
    }
    for (int tile = blockIdx.x; tile * TILE < total; tile += gridDim.x) {
        const int j0 = tile * TILE, tid = opaque(threadIdx.x);
        if (tid < TILE * LDO) {
            const int s = tid / LDO, c = tid % LDO, j = j0 + s;
            const bool live = j < total;
            int64_t row = 0;
            if (live) row = a.rng_state ? (int64_t)perm_row(sample_base_at(seed, counter + (uint64_t)(j / a.batch)), (uint32_t)a.ring_size, (uint32_t)(j % a.batch)) : a.idx[j];
            S[S_NOBS + s * LDO + c] = (live && c < OBS) ? a.next_states[row * OBS + c] : 0.f;
            if (c == 0 && live) {      // r and done wait in the gradient buffer, which the forward leaves alone
                S[S_D0 + s] = a.rewards[row];
                S[S_D0 + TILE + s] = a.dones[row];
            }
        }
        __syncthreads();
        float rew = 0.f, done = 0.f;
        if (tid < TILE && j0 + tid < total) { rew = S[S_D0 + tid]; done = S[S_D0 + TILE + tid]; }
        forward(a.target, S + S_NOBS, S, tid);
        if (tid < TILE && j0 + tid < total) {
            float mx = S[S_Q + tid * LDA];
            for (int j = 1; j < A; ++j) mx = fmaxf(mx, S[S_Q + tid * LDA + j]);
            const float t = (1.f - done) * a.gamma;
            y[j0 + tid] = rew + t * mx;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(THREADS) void dqn_multi_target_kernel(const DqnStepsArgs a) {
    dqn_multi_target_body(a);
}

// The chain: ONE workgroup of ceil(batch / 16) groups of 512 threads, group g carrying batch slots [16 g, 16 g + 16) through every step.
struct ChainGroup {      // a thread's view of its group; asked for anew in every phase of a step, so that nothing of it lives across the phases
    int tid, lt, grp, slot0;
    float *S;
    int *s_act;
    float *part;
};
__device__ __forceinline__ ChainGroup chain_group(float *S_all, int *s_act_all, float *ws) {
    ChainGroup g;
    g.tid = opaque(threadIdx.x);
    g.lt = ltid_of(g.tid);
    g.grp = __builtin_amdgcn_readfirstlane(g.tid / THREADS);      // (a wave lies in one group)
    g.slot0 = g.grp * TILE;
    g.S = S_all + g.grp * S_TOTAL;
    g.s_act = s_act_all + g.grp * TILE;
    g.part = ws + (int64_t)g.grp * P_PAD;
    return g;
}

// (The body of dqn_multi_chain_kernel and of its grouped form, where one workgroup per learner runs it on that learner's buffers.)
__device__ __forceinline__ void dqn_multi_chain_body(const DqnStepsArgs &a) {
    __shared__ __attribute__((aligned(16))) float S_all[CHAIN_TILES * S_TOTAL];
    __shared__ int s_act_all[CHAIN_TILES * TILE];
    __shared__ float s_red[WAVES];
    __shared__ float s_part_loss[CHAIN_TILES];
    __shared__ float s_coef;
    const int n_part = blockDim.x / THREADS, n_threads = blockDim.x;
    const float *y = a.ws + ms_y(), *adam = a.ws + ms_adam(a.n_steps);
    const uint64_t seed = a.rng_state ? a.rng_state[0] : 0, counter = a.rng_state ? a.rng_state[1] : 0;
    const int step0 = *a.step;

    for (int k = 0; k < a.n_steps; ++k) {
        {   // ---- this group's 16 transitions of step k and their TD targets (slots past the batch: zero observations, no gradient)
            const ChainGroup g = chain_group(S_all, s_act_all, a.ws);
            float *S = g.S;
            if (g.lt < TILE * LDO) {
                const int s = g.lt / LDO, c = g.lt % LDO, b = g.slot0 + s;
                const bool live = b < a.batch;
                int64_t row = 0;
                if (live) row = a.rng_state ? (int64_t)perm_row(sample_base_at(seed, counter + (uint64_t)k), (uint32_t)a.ring_size, (uint32_t)b) : a.idx[k * a.batch + b];
                S[S_OBS + s * LDO + c] = (live && c < OBS) ? a.states[row * OBS + c] : 0.f;
                if (c == 0) {
                    int64_t act = live ? a.actions[row] : 0;
                    g.s_act[s] = (act >= 0 && act < A) ? (int)act : 0;
                    if (live && a.idx_out) a.idx_out[k * a.batch + b] = row;
                    S[S_Y + s] = live ? y[k * a.batch + b] : 0.f;
                }
            }
        }
        __syncthreads();
        {   // ---- local forward, loss, dL/dQ
            const ChainGroup g = chain_group(S_all, s_act_all, a.ws);
            float *S = g.S;
            const int lt = g.lt;
            forward(a.params, S + S_OBS, S, g.tid);
            if (lt < TILE) {
                const bool live = g.slot0 + lt < a.batch;
                const float d = S[S_Q + lt * LDA + g.s_act[lt]] - S[S_Y + lt];
                const float ad = fabsf(d);
                const float term = ad < 1.f ? 0.5f * d * d : ad - 0.5f;       // smooth_l1, beta = 1
                const float gq = (ad < 1.f ? d : copysignf(1.f, d)) * a.inv_batch;
                for (int j = 0; j < LDA; ++j) S[S_D0 + lt * LDD + j] = (live && j == g.s_act[lt]) ? gq : 0.f;
                S[S_Y + lt] = live ? term : 0.f;
            }
            __syncthreads();
            if (lt == 0) {
                float t = 0.f;
                for (int s = 0; s < TILE; ++s) t += S[S_Y + s];
                s_part_loss[g.grp] = t;
            }
        }
        // ---- backward, output layer first; D0 / D1 alternate as dY and dX
#define CHAIN_BWD(K_, N_, DX_, MASK_, dY_, X_, ldx_, OW_, OB_, dX_)                                                                          \
    {                                                                                                                                        \
        const ChainGroup g = chain_group(S_all, s_act_all, a.ws);                                                                            \
        float *S = g.S;                                                                                                                      \
        bwd_layer<K_, N_, DX_, MASK_>(S + (dY_), S + (X_), ldx_, a.params + OW_, g.part + OW_, g.part + OB_, S + (dX_), g.tid);              \
    }
        CHAIN_BWD(H, A, true, true, S_D0, S_Q2, LDH, O_Q4W, O_Q4B, S_D1)      // q_net.4
        __syncthreads();
        CHAIN_BWD(H, H, true, true, S_D1, S_Q1, LDH, O_Q2W, O_Q2B, S_D0)      // q_net.2
        __syncthreads();
        CHAIN_BWD(A, H, true, false, S_D0, S_O, LDA, O_Q0W, O_Q0B, S_D1)      // q_net.0
        __syncthreads();
        CHAIN_BWD(H, A, true, true, S_D1, S_H2, LDH, O_OW, O_OB, S_D0)        // output_layer
        __syncthreads();
        CHAIN_BWD(H, H, true, true, S_D0, S_H1, LDH, O_H2W, O_H2B, S_D1)      // hidden_layer_2
        __syncthreads();
        CHAIN_BWD(F, H, true, false, S_D1, S_F, LDF, O_HW, O_HB, S_D0)        // hidden_layer
        __syncthreads();
        CHAIN_BWD(2, 16, false, false, S_D0, S_OBS, LDO, O_VW, O_VB, 0)       // encoders (no dX: the last two arguments are unused)
        CHAIN_BWD(2, 16, false, false, S_D0 + 16, S_OBS + 2, LDO, O_GW, O_GB, 0)
        CHAIN_BWD(22, 176, false, false, S_D0 + 32, S_OBS + 4, LDO, O_SW, O_SB, 0)
#undef CHAIN_BWD
        chain_handoff();      // the rows: written by every group, summed by the first

        // ---- gradient = sum of the rows in index order, its squared norm on the single step's 512-thread mapping
        {
            const int tid = opaque(threadIdx.x);
            if (tid < THREADS) {
                float sq = 0.f;
                for (int q = tid; q < P_PAD / 4; q += THREADS) {
                    float4 g = reinterpret_cast<const float4 *>(a.ws)[q];
                    for (int w = 1; w < n_part; ++w) {
                        const float4 x = reinterpret_cast<const float4 *>(a.ws + (int64_t)w * P_PAD)[q];
                        g.x += x.x; g.y += x.y; g.z += x.z; g.w += x.w;
                    }
                    const float e[4] = {g.x, g.y, g.z, g.w};
                    float e2[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int p = 4 * q + c;
                        e2[c] = p < P_TOTAL ? e[c] : 0.f;
                        if (p < P_TOTAL) a.grad[p] = e[c];
                    }
                    sq += sumsq4(e2[0], e2[1], e2[2], e2[3]);
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) sq += shfl_xor_of(sq, off, tid);
                if (lane_of(tid) == 0) s_red[wave_of(tid)] = sq;
            }
            __syncthreads();
            if (tid == 0) {
                float tot = 0.f;
                for (int w = 0; w < WAVES; ++w) tot += s_red[w];
                const float norm = sqrtf(tot);
                s_coef = fminf((float)a.max_norm / (norm + 1e-6f), 1.f);      // clip_grad_norm_: coef = max_norm / (norm + 1e-6), clamped to 1
                float l = 0.f;
                for (int w = 0; w < n_part; ++w) l += s_part_loss[w];
                a.loss[k] = l / a.batch_f;
            }
        }
        chain_handoff();      // the gradient: written on the 512-thread mapping, clipped and applied by every lane
        {   // ---- clip + Adam, element-wise over all lanes
            const int tid = opaque(threadIdx.x);
            const float coef = s_coef, step_size = adam[2 * k], bc2_sqrt = adam[2 * k + 1];
            for (int q = tid; q < P_PAD / 4; q += n_threads)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int p = 4 * q + c;
                    if (p >= P_TOTAL) continue;
                    const float gq = a.grad[p] * coef;
                    a.grad[p] = gq;
                    float mm = a.m[p], vv = a.v[p], pp = a.params[p];
                    adam_update(gq, mm, vv, pp, a.w1, a.b2f, a.w2, step_size, bc2_sqrt, a.eps_f);
                    a.m[p] = mm;
                    a.v[p] = vv;
                    a.params[p] = pp;
                }
        }
        chain_handoff();      // the parameters (and the moments): the next step's forward must not be served this step's lines
    }
    if (threadIdx.x == 0) {
        *a.step = step0 + a.n_steps;
        if (a.rng_state) a.rng_state[1] = counter + (uint64_t)a.n_steps;
    }
}

__global__ __launch_bounds__(CHAIN_THREADS) void dqn_multi_chain_kernel(const DqnStepsArgs a) {
    dqn_multi_chain_body(a);
}


// ---- many learners per launch (mn_dqn_group_*) -----------------------------------------------------------------------------------------------------------
// G independent learners with common hyper-parameters in one launch: the learner is a grid dimension.  Workgroup (w, g) of dqn_train_step_groups_kernel IS
// workgroup w of learner g's dqn_train_step_kernel -- the same body on g's own ring, networks, moments, counters and its own slice of the workspace (rows,
// partial losses, ticket) -- and likewise for the two kernels of the multi-step call.  No learner reads what another writes, so each is bit for bit what it
// is when launched alone.  The learners' pointers come from a device-resident table: the row address is wave-uniform, the loads are scalar and the pointers
// sit where the kernel arguments of the single forms sit, in scalar registers.
struct DqnLearnerRow {      // mn_dqn_learner with the kernels' names
    const float *states, *next_states;
    const int64_t *actions;
    const float *rewards, *dones;
    uint64_t *rng_state;
    float *params;
    const float *target;
    float *grad, *m, *v;
    int32_t *step;
};

struct DqnGroupArgs {      // what a call has in common for the group; idx / idx_out: [G][n_steps][batch] or NULL; loss: [G][n_steps]; ws: [G][ws_stride]
    const DqnLearnerRow *table;
    int64_t ring_size;
    const int64_t *idx;
    int64_t *idx_out;
    float *ws;
    int64_t ws_stride;
    float *loss;
    int batch;
    float gamma;
    double lr, b1, b2, eps, max_norm;
    int n_steps;      // 1 for the single step
    float w1, b2f, w2, eps_f, batch_f, inv_batch;      // as DqnStepsArgs
};

// learner g's arguments of the single form
__device__ __forceinline__ void learner_args(DqnTrainArgs &a, const DqnGroupArgs &ga, int g) {
    const DqnLearnerRow r = ga.table[g];
    const int64_t rows = (int64_t)g * ga.n_steps * ga.batch;
    a.states = r.states; a.next_states = r.next_states; a.actions = r.actions; a.rewards = r.rewards; a.dones = r.dones;
    a.ring_size = ga.ring_size;
    a.rng_state = ga.idx ? nullptr : r.rng_state;      // given rows: the draw state is left alone, as in the single calls
    a.idx = ga.idx ? ga.idx + rows : nullptr;
    a.idx_out = ga.idx_out ? ga.idx_out + rows : nullptr;
    a.params = r.params; a.target = r.target; a.grad = r.grad; a.m = r.m; a.v = r.v; a.step = r.step;
    a.ws = ga.ws + (int64_t)g * ga.ws_stride;
    a.loss = ga.loss + (int64_t)g * ga.n_steps;
    a.batch = ga.batch; a.gamma = ga.gamma; a.lr = ga.lr; a.b1 = ga.b1; a.b2 = ga.b2; a.eps = ga.eps; a.max_norm = ga.max_norm;
}

__device__ __forceinline__ void learner_steps_args(DqnStepsArgs &a, const DqnGroupArgs &ga, int g) {
    learner_args(a, ga, g);
    a.n_steps = ga.n_steps;
    a.w1 = ga.w1; a.b2f = ga.b2f; a.w2 = ga.w2; a.eps_f = ga.eps_f; a.batch_f = ga.batch_f; a.inv_batch = ga.inv_batch;
}

__global__ __launch_bounds__(THREADS) void dqn_train_step_groups_kernel(const DqnGroupArgs ga) {      // grid (ceil(batch / 16), G)
    DqnTrainArgs a;
    learner_args(a, ga, blockIdx.y);
    dqn_train_step_body(a);
}

__global__ __launch_bounds__(THREADS) void dqn_multi_target_groups_kernel(const DqnGroupArgs ga) {      // grid (tiles, G)
    DqnStepsArgs a;
    learner_steps_args(a, ga, blockIdx.y);
    dqn_multi_target_body(a);
}

__global__ __launch_bounds__(CHAIN_THREADS) void dqn_multi_chain_groups_kernel(const DqnGroupArgs ga) {      // grid (G): workgroup g is learner g's whole chain
    DqnStepsArgs a;
    learner_steps_args(a, ga, blockIdx.x);
    dqn_multi_chain_body(a);
}

__host__ constexpr int64_t round4(int64_t n) { return (n + 3) & ~(int64_t)3; }

// [lo, hi) byte extents overlap
bool overlap(const void *p, size_t np, const void *q, size_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + nq && b < a + np;
}

}  // namespace

struct mn_dqn_group {
    DqnLearnerRow *table_dev;
    int n;
    bool all_draw;      // every learner has a draw state
};

extern "C" int mn_dqn_group_create(const mn_dqn_learner *learners_host, int32_t n_learners, mn_dqn_group **out) {
    if (!out) return MN_ERR_INVALID;
    *out = nullptr;
    if (!learners_host || n_learners < 1 || n_learners > MN_DQN_MAX_LEARNERS) return MN_ERR_INVALID;
    DqnLearnerRow rows[MN_DQN_MAX_LEARNERS];
    struct Extent { const void *p; size_t n; int owner; };
    Extent written[6 * MN_DQN_MAX_LEARNERS], targets[MN_DQN_MAX_LEARNERS];
    int n_written = 0;
    bool all_draw = true;
    constexpr size_t VEC = (size_t)P_TOTAL * sizeof(float);
    for (int g = 0; g < n_learners; ++g) {
        const mn_dqn_learner &l = learners_host[g];
        if (!l.ring_states || !l.ring_next_states || !l.ring_actions || !l.ring_rewards || !l.ring_dones || !l.params_local || !l.params_target || !l.grad ||
            !l.exp_avg || !l.exp_avg_sq || !l.step)
            return MN_ERR_INVALID;
        rows[g] = DqnLearnerRow{l.ring_states, l.ring_next_states, l.ring_actions, l.ring_rewards, l.ring_dones, l.rng_state, l.params_local, l.params_target,
                                l.grad, l.exp_avg, l.exp_avg_sq, l.step};
        written[n_written++] = Extent{l.params_local, VEC, g};
        written[n_written++] = Extent{l.grad, VEC, g};
        written[n_written++] = Extent{l.exp_avg, VEC, g};
        written[n_written++] = Extent{l.exp_avg_sq, VEC, g};
        written[n_written++] = Extent{l.step, sizeof(int32_t), g};
        if (l.rng_state) written[n_written++] = Extent{l.rng_state, 2 * sizeof(uint64_t), g};
        else all_draw = false;
        targets[g] = Extent{l.params_target, VEC, g};
    }
    // learners that alias would race silently: nothing one learner writes may overlap what another writes, or the target network another reads
    for (int i = 0; i < n_written; ++i) {
        for (int j = i + 1; j < n_written; ++j)
            if (written[i].owner != written[j].owner && overlap(written[i].p, written[i].n, written[j].p, written[j].n)) return MN_ERR_INVALID;
        for (int g = 0; g < n_learners; ++g)
            if (written[i].owner != g && overlap(written[i].p, written[i].n, targets[g].p, targets[g].n)) return MN_ERR_INVALID;
    }
    mn_dqn_group *grp = new (std::nothrow) mn_dqn_group{nullptr, n_learners, all_draw};
    if (!grp) return MN_ERR_HIP;
    if (hipMalloc(&grp->table_dev, sizeof(DqnLearnerRow) * n_learners) != hipSuccess ||
        hipMemcpy(grp->table_dev, rows, sizeof(DqnLearnerRow) * n_learners, hipMemcpyHostToDevice) != hipSuccess) {
        if (grp->table_dev) (void)hipFree(grp->table_dev);
        delete grp;
        return MN_ERR_HIP;
    }
    *out = grp;
    return MN_OK;
}

extern "C" int mn_dqn_group_destroy(mn_dqn_group *g) {
    if (!g) return MN_ERR_INVALID;
    const hipError_t e = hipFree(g->table_dev);
    delete g;
    return e == hipSuccess ? MN_OK : MN_ERR_HIP;
}

namespace {

// the checks and the kernel arguments the two grouped calls share (n_steps 1: the single step); the caller sets ws_stride
int group_args(DqnGroupArgs &ga, const mn_dqn_group *g, int64_t ring_size, const int64_t *idx_dev, int64_t *idx_out, float *workspace, float *losses_out,
               int32_t batch, int32_t max_batch, int32_t n_steps, float gamma, double lr, double beta1, double beta2, double eps, double max_norm) {
    if (!g || !workspace || !losses_out) return MN_ERR_INVALID;
    if (batch <= 0 || batch > max_batch || n_steps < 1 || n_steps > MAX_STEPS) return MN_ERR_INVALID;
    if (ring_size < batch || ring_size > 0x7fffffff) return MN_ERR_INVALID;
    if (!idx_dev && !g->all_draw) return MN_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return MN_ERR_INVALID;
    ga.table = g->table_dev; ga.ring_size = ring_size; ga.idx = idx_dev; ga.idx_out = idx_out; ga.ws = workspace; ga.loss = losses_out;
    ga.batch = batch; ga.gamma = gamma; ga.lr = lr; ga.b1 = beta1; ga.b2 = beta2; ga.eps = eps; ga.max_norm = max_norm; ga.n_steps = n_steps;
    ga.w1 = (float)(1.0 - beta1); ga.b2f = (float)beta2; ga.w2 = (float)(1.0 - beta2); ga.eps_f = (float)eps;
    ga.batch_f = (float)batch; ga.inv_batch = 1.f / (float)batch;
    return MN_OK;
}

}  // namespace

extern "C" int mn_dqn_group_train_step(mn_dqn_group *g, int64_t ring_size, const int64_t *idx_dev, int64_t *idx_out, float *workspace, float *losses_out,
                                       int32_t batch, float gamma, double lr, double beta1, double beta2, double eps, double max_norm, void *stream) {
    DqnGroupArgs ga;
    const int rc = group_args(ga, g, ring_size, idx_dev, idx_out, workspace, losses_out, batch, MAX_BATCH_DQN, 1, gamma, lr, beta1, beta2, eps, max_norm);
    if (rc != MN_OK) return rc;
    const int n_part = (batch + TILE - 1) / TILE;
    ga.ws_stride = round4(ws_total(n_part));
    hipLaunchKernelGGL(dqn_train_step_groups_kernel, dim3(n_part, g->n), dim3(THREADS), 0, (hipStream_t)stream, ga);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

extern "C" int mn_dqn_group_train_steps(mn_dqn_group *g, int64_t ring_size, const int64_t *idx_dev, int64_t *idx_out, float *workspace, float *losses_out,
                                        int32_t batch, int32_t n_steps, float gamma, double lr, double beta1, double beta2, double eps, double max_norm,
                                        void *stream) {
    DqnGroupArgs ga;
    const int rc = group_args(ga, g, ring_size, idx_dev, idx_out, workspace, losses_out, batch, CHAIN_BATCH, n_steps, gamma, lr, beta1, beta2, eps, max_norm);
    if (rc != MN_OK) return rc;
    ga.ws_stride = round4(ms_total(n_steps));
    const int tiles = (n_steps * batch + TILE - 1) / TILE, n_part = (batch + TILE - 1) / TILE;
    hipLaunchKernelGGL(dqn_multi_target_groups_kernel, dim3(tiles < 1024 ? tiles : 1024, g->n), dim3(THREADS), 0, (hipStream_t)stream, ga);
    hipLaunchKernelGGL(dqn_multi_chain_groups_kernel, dim3(g->n), dim3(n_part * THREADS), 0, (hipStream_t)stream, ga);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

extern "C" int64_t mn_dqn_train_workspace_floats(int32_t batch) {
    if (batch <= 0 || batch > MAX_BATCH_DQN) return -1;
    return ws_total((batch + TILE - 1) / TILE);
}

extern "C" int mn_dqn_train_step(const float *ring_states, const float *ring_next_states, const int64_t *ring_actions, const float *ring_rewards,
                                 const float *ring_dones, int64_t ring_size, uint64_t *rng_state_dev, const int64_t *idx_dev, int64_t *idx_out,
                                 float *params_local, const float *params_target, float *workspace, float *grad_out, float *loss_out, float *exp_avg,
                                 float *exp_avg_sq, int32_t *step_dev, int32_t batch, float gamma, double lr, double beta1, double beta2, double eps,
                                 double max_norm, void *stream) {
    if (!ring_states || !ring_next_states || !ring_actions || !ring_rewards || !ring_dones || !params_local || !params_target || !workspace ||
        !grad_out || !loss_out || !exp_avg || !exp_avg_sq || !step_dev)
        return MN_ERR_INVALID;
    if (batch <= 0 || batch > MAX_BATCH_DQN) return MN_ERR_INVALID;
    if (rng_state_dev) {
        if (ring_size < batch || ring_size > 0x7fffffff) return MN_ERR_INVALID;
    } else if (!idx_dev) {
        return MN_ERR_INVALID;
    }
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return MN_ERR_INVALID;
    DqnTrainArgs a;
    a.states = ring_states; a.next_states = ring_next_states; a.actions = ring_actions; a.rewards = ring_rewards; a.dones = ring_dones;
    a.ring_size = ring_size; a.rng_state = rng_state_dev; a.idx = idx_dev; a.idx_out = idx_out;
    a.params = params_local; a.target = params_target; a.ws = workspace; a.grad = grad_out; a.loss = loss_out; a.m = exp_avg; a.v = exp_avg_sq;
    a.step = step_dev; a.batch = batch; a.gamma = gamma; a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.max_norm = max_norm;
    hipLaunchKernelGGL(dqn_train_step_kernel, dim3((batch + TILE - 1) / TILE), dim3(THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

extern "C" int64_t mn_dqn_train_steps_workspace_floats(int32_t batch, int32_t n_steps) {
    if (batch <= 0 || batch > CHAIN_BATCH || n_steps <= 0 || n_steps > MAX_STEPS) return -1;
    return ms_total(n_steps);
}

// parts: 1 = the TD targets and Adam scalars of every step, 2 = the chain (on the targets a part-1 call left in the workspace), 3 = both
extern "C" int mn_dqn_train_steps_parts(const float *ring_states, const float *ring_next_states, const int64_t *ring_actions, const float *ring_rewards,
                                        const float *ring_dones, int64_t ring_size, uint64_t *rng_state_dev, const int64_t *idx_dev, int64_t *idx_out,
                                        float *params_local, const float *params_target, float *workspace, float *grad_out, float *losses_out,
                                        float *exp_avg, float *exp_avg_sq, int32_t *step_dev, int32_t batch, int32_t n_steps, float gamma, double lr,
                                        double beta1, double beta2, double eps, double max_norm, int32_t parts, void *stream) {
    if (!ring_states || !ring_next_states || !ring_actions || !ring_rewards || !ring_dones || !params_local || !params_target || !workspace ||
        !grad_out || !losses_out || !exp_avg || !exp_avg_sq || !step_dev)
        return MN_ERR_INVALID;
    if (batch <= 0 || batch > CHAIN_BATCH || n_steps <= 0 || n_steps > MAX_STEPS || parts < 1 || parts > 3) return MN_ERR_INVALID;
    if (rng_state_dev) {
        if (ring_size < batch || ring_size > 0x7fffffff) return MN_ERR_INVALID;
    } else if (!idx_dev) {
        return MN_ERR_INVALID;
    }
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return MN_ERR_INVALID;
    DqnStepsArgs a;
    a.states = ring_states; a.next_states = ring_next_states; a.actions = ring_actions; a.rewards = ring_rewards; a.dones = ring_dones;
    a.ring_size = ring_size; a.rng_state = rng_state_dev; a.idx = idx_dev; a.idx_out = idx_out;
    a.params = params_local; a.target = params_target; a.ws = workspace; a.grad = grad_out; a.loss = losses_out; a.m = exp_avg; a.v = exp_avg_sq;
    a.step = step_dev; a.batch = batch; a.gamma = gamma; a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.max_norm = max_norm;
    a.n_steps = n_steps;
    a.w1 = (float)(1.0 - beta1); a.b2f = (float)beta2; a.w2 = (float)(1.0 - beta2); a.eps_f = (float)eps;
    a.batch_f = (float)batch; a.inv_batch = 1.f / (float)batch;
    const int tiles = (n_steps * batch + TILE - 1) / TILE, n_part = (batch + TILE - 1) / TILE;
    if (parts & 1) hipLaunchKernelGGL(dqn_multi_target_kernel, dim3(tiles < 1024 ? tiles : 1024), dim3(THREADS), 0, (hipStream_t)stream, a);
    if (parts & 2) hipLaunchKernelGGL(dqn_multi_chain_kernel, dim3(1), dim3(n_part * THREADS), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

extern "C" int mn_dqn_train_steps(const float *ring_states, const float *ring_next_states, const int64_t *ring_actions, const float *ring_rewards,
                                  const float *ring_dones, int64_t ring_size, uint64_t *rng_state_dev, const int64_t *idx_dev, int64_t *idx_out,
                                  float *params_local, const float *params_target, float *workspace, float *grad_out, float *losses_out, float *exp_avg,
                                  float *exp_avg_sq, int32_t *step_dev, int32_t batch, int32_t n_steps, float gamma, double lr, double beta1, double beta2,
                                  double eps, double max_norm, void *stream) {
    return mn_dqn_train_steps_parts(ring_states, ring_next_states, ring_actions, ring_rewards, ring_dones, ring_size, rng_state_dev, idx_dev, idx_out,
                                    params_local, params_target, workspace, grad_out, losses_out, exp_avg, exp_avg_sq, step_dev, batch, n_steps, gamma, lr,
                                    beta1, beta2, eps, max_norm, 3, stream);
}
