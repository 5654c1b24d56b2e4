// mn_rollout_iqn_body.h -- one IQN evaluation episode per wavefront: the body of the IQN episode launches.
// Included ONCE by mn_rollout_iqn.hip (QUANT = false: the acting form, mn_rollout_iqn / mn_rollout_iqn_rows), by mn_rollout_iqn_eval.hip
// (QUANT = true: act_eval's form, which also records the quantile values and taus each action was chosen from, mn_rollout_iqn_eval) and by
// mn_rollout_iqn_groups.hip (the acting form with GROUPED = true: every group of rows its own weight image and tau stream, mn_rollout_iqn_groups);
// each wraps iqn_episode<> in its own __global__ kernel.  All three files are built with -ffp-contract=fast-honor-pragmas (Makefile).
//
// Floating-point contraction: the network is built like iqn_act.o (contraction allowed -- fast-honor-pragmas without a pragma compiles the
// per-row act kernels to the same code as -ffp-contract=fast), the step body and adjust_cvar under `#pragma clang fp contract(off)`, like
// the env kernels (mn_step.o / mn_rollout.o are built with -ffp-contract=off; the pragma reproduces that code object exactly).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>

#include "marinenav_hip.h"

#pragma clang fp contract(off)
#include "mn_step_body.h"

namespace {

// IQNAgent.adjust_cvar_batch (agent.py) for one float32 observation row, bitwise as PyTorch on ROCm computes it: the norm of each sonar point
// is linalg.vector_norm's reduction -- the two squares rounded separately (two accumulators), their sum rounded, a correctly rounded square
// root --; points with both coordinates below 1e-3 are skipped; `closest / 10.0` runs as a multiplication by the float32 reciprocal 0.1f
// (the division by a CPU scalar).  Contraction is off here: every operation rounds on its own.
__device__ __forceinline__ float adjust_cvar_row(const float *row) {
    float closest = INFINITY;
#pragma unroll
    for (int b = 0; b < MN_NUM_BEAMS; ++b) {
        const float px = row[4 + 2 * b], py = row[5 + 2 * b];
        const float xx = px * px, yy = py * py;
        const float d = (float)__builtin_sqrt((double)(xx + yy));      // (the float64 root of a float32 rounds correctly to float32)
        const bool skip = fabsf(px) < 1e-3f && fabsf(py) < 1e-3f;
        closest = fminf(closest, skip ? INFINITY : d);
    }
    return closest < 10.0f ? closest * (1.0f / 10.0f) : 1.0f;
}

}  // namespace

#pragma clang fp contract(fast)

namespace {

#include "iqn_act_common.h"
#include "iqn_act_split.h"

struct IqnTrace {
    float *obs;        // [T][n][26] observation each step returned (not written once the env has finished)
    float *reward;     // [T][n]     0 once finished
    uint8_t *done;     // [T][n]     1 once finished
    uint8_t *info;     // [T][n]     the terminal code once finished
    int32_t *action;   // [T][n]     -1 once finished
    float *cvar;       // [T][n]     the cvar the step's taus were drawn with (not written once finished)
    float *q;          // [T][n][9]  Q(s, .) the action was chosen from (not written once finished)
    double *traj;      // [T][n][N][2] the step's sub-step positions (mn_set_trajectory_trace; float64 handles; not written once finished)
    float *quantiles;  // [T][n][32][9] QUANT only: the quantile values Z(tau, a) the action was chosen from (not written once finished)
    float *taus;       // [T][n][32]    QUANT only: the taus they belong to (not written once finished)
};

// LDS of one episode wavefront: the weight image -- the acting image, or with QUANT the full one incl. the output layer's MFMA operands --, behind it
// the wave's feature buffer and the observation row; NOISE: behind that the row the robot perceives (mn_set_obs_noise)
template <bool QUANT, bool NOISE = false> struct IqnLds {
    static constexpr int IMG = QUANT ? sp::OFF_FB : sp::ACT_IMG_FLOATS;
    static constexpr int ROW_OFF = IMG + F;
    static constexpr int SEEN_OFF = ROW_OFF + 32;
    static constexpr int FLOATS = ROW_OFF + (NOISE ? 64 : 32);
    static_assert(IMG % 4 == 0 && ROW_OFF % 4 == 0, "16-byte aligned feature buffer and row");
    static_assert(FLOATS * 4 <= 160 * 1024, "fits the CU's 160 KB");
};

// Which rows of a launch act together (GROUPED = true): row e belongs to group e / rows and is row e % rows of it.  A group has its own weight image
// (packed + group * stride), its own {seed, counter} (rng_state + 2 * group), its own ticket and maximum (words + 2 * group) and its own steps_out entry,
// and keys its tau draws by the row's index INSIDE the group: it draws, and leaves in its counter, what a launch of its own on `rows` rows does.
// GROUPED = false: one group, the whole launch -- the descriptor is not read.
struct IqnGroups {
    int rows;          // rows per group
    int64_t stride;    // 32-bit words from one group's weight image to the next (a multiple of 4: the image is staged 16 bytes at a time)
};

// QUANT = false: Q as the acting form of iqn_qvals_split_kernel computes it (tau mean before the f32 output layer: mn_iqn_act_rng without quantiles_dev).
// QUANT = true : as its QUANT = true form (per-tau output layer on the matrix pipe, Q = the mean of those values: mn_iqn_act_rng with quantiles_dev,
//                IQNAgent.act_eval) -- the two can differ in the last bit -- and T.quantiles / T.taus are recorded.
// NOISE (mn_set_obs_noise): at the head of a step lanes 0 .. 14 fill the perceived row, one channel each, from the clean row under the key (seed, global
//                env index, the env's ep_t); adjust_cvar_row and the encoder read THAT row -- the robot adapts its CVaR to what it perceives -- while the
//                step keeps writing the clean one: obs_io, the traces and the act call counter are what they are without noise.  NOISE = false is the
//                body as it was; `NS` is not read.
template <typename M, bool PARITY, int L, bool QUANT, bool GROUPED = false, bool NOISE = false>
__device__ __forceinline__ void iqn_episode(float *lds, MnArrays A, const MnDev &P, int n_steps, const uint32_t *__restrict__ packed, uint64_t *rng_state,
                                            float cvar, int adaptive, const float *__restrict__ cvar_row, const uint8_t *__restrict__ adaptive_row,
                                            float *__restrict__ obs_io, const IqnTrace &T, uint32_t *__restrict__ words, int32_t *__restrict__ steps_out,
                                            const IqnGroups &G, const MnObsNoiseArg &NS = MnObsNoiseArg{}) {
    using namespace sp;
    using Lds = IqnLds<QUANT, NOISE>;
    using Lane = MnLane<M, PARITY, L>;
    const int lane = threadIdx.x, g = lane >> 4, col = lane & 15;
    const int e = blockIdx.x;
    const size_t n = (size_t)A.n;
    if (e == 0 && lane < 2 * MN_QSHARDS) A.queue_count[lane * MN_QSTRIDE] = 0u;   // nothing is left for a later mn_reset_done
    int draw_row = e;                     // the row index the tau draws are keyed with
    if constexpr (GROUPED) {
        const int grp = e / G.rows;
        draw_row = e - grp * G.rows;
        packed += (size_t)grp * (size_t)G.stride;
        rng_state += 2 * (size_t)grp;
        words += 2 * (size_t)grp;
        if (steps_out) steps_out += grp;
    }
    const uint64_t seed = rng_state[0], ctr0 = rng_state[1];
    // per-env cvar / adaptive flag (one env per wavefront: wave-uniform loads, outside the step loop); NULL = the launch's scalar
    if (cvar_row) cvar = cvar_row[e];
    if (adaptive_row) adaptive = adaptive_row[e];

    {   // the weight image (iqn_qvals_split_kernel's IMG for this QUANT)
        const u32x4 *src = reinterpret_cast<const u32x4 *>(packed);
        u32x4 *dst = reinterpret_cast<u32x4 *>(lds);
        for (int i = lane; i < Lds::IMG / 4; i += MN_WAVE) dst[i] = src[i];
    }
    float *row = lds + Lds::ROW_OFF;
    for (int k = lane; k < MN_OBS_DIM; k += MN_WAVE) row[k] = obs_io[(size_t)e * MN_OBS_DIM + k];     // the observation the episode continues from

    const f32x4 *ldsv = reinterpret_cast<const f32x4 *>(lds);
    const u32x4 *lds4 = reinterpret_cast<const u32x4 *>(lds);
    LdsBase lb;
    lb.w_lo = lane; lb.w_hi = lane + 4096; lb.fl = (OFF_B1 >> 2) + g; lb.fb = (Lds::IMG >> 2) + g;
    int enc_w = (OFF_WS >> 2) + lane, enc_f = OFF_BND + lane, fb_f = Lds::IMG + lane;
    asm volatile("" : "+v"(lb.w_lo), "+v"(lb.w_hi), "+v"(lb.fl), "+v"(lb.fb), "+v"(enc_w), "+v"(enc_f), "+v"(fb_f));
    __syncthreads();
    const float c1 = lds[OFF_CST + 0], c2 = lds[OFF_CST + 1], c3 = lds[OFF_CST + 2];
    const float a2 = lds[OFF_CST + 3], d2 = lds[OFF_CST + 4], a3 = lds[OFF_CST + 5], d3 = lds[OFF_CST + 6];
    const float hk0 = 4.0f * (float)g;

    const MnRing none = {};
    Lane ln;
    ln.load(A, e, lane % L);
    ln.active = ln.active && lane < L;      // group 0 writes; the other groups compute the same environment
    int steps = n_steps, last_info = 0;
    for (int t = 0; t < n_steps; ++t) {
        __syncthreads();      // the row of the previous step is complete
        // ---- act: mn_iqn_act_rng's draws and split-f16 forward pass for this row (call counter ctr0 + t, eps = 0)
        const float *prow = row;      // the row the policy reads
        if constexpr (NOISE) {
            float *seen = lds + Lds::SEEN_OFF;
            const uint64_t key = mn_obs_noise_row_key(NS.S.seed, NS.env0 + (uint64_t)e, (uint64_t)(int64_t)__builtin_amdgcn_readfirstlane(ln.ep_t));
            if (lane < MN_OBS_NOISE_CHANNELS) mn_obs_noise_channel(row, seen, lane, key, NS.S);
            __syncthreads();      // the perceived row is complete
            prow = seen;
        }
        const float cv = adaptive ? adjust_cvar_row(prow) : cvar;
        uint32_t k0, k1;
        draw_keys(seed, ctr0 + (uint64_t)t, k0, k1);
        float tau[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) tau[nt] = tau_draw(draw_row, 16 * nt + col, k0, k1, cv);
        f16x8 cbh[2][NT], cbl[2][NT];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                f16x2 h[4], l[4];
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    split2(__builtin_amdgcn_cosf(tau[nt] * (hk0 + (16.0f * kb + 0.5f * (2 * p)))),
                           __builtin_amdgcn_cosf(tau[nt] * (hk0 + (16.0f * kb + 0.5f * (2 * p + 1)))), h[p], l[p]);
                cbh[kb][nt] = cat4(h[0], h[1], h[2], h[3]);
                cbl[kb][nt] = cat4(l[0], l[1], l[2], l[3]);
            }
        float ov[28];
#pragma unroll
        for (int i = 0; i < 28; ++i) ov[i] = i < OBS ? prow[i] : 0.f;
        const EnvScale sc = encode_env<false>(lds, ldsv, enc_w, enc_f, fb_f, lane, ov, c1, a2, d2, a3, d3);
        CosJob cj;      // (no next environment: its pieces inside stage 5 / the tail are dead code)
        cj.hk0 = hk0; cj.tau[0] = cj.tau[1] = 0.f;
        f32x4 acc2[4][NT], acc3[4][NT];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc2[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        f16x8 bhA[NT], blA[NT], bhB[NT], blB[NT];
        f32x4 accA[2][NT], accB[2][NT];
        stage<-2>(lds4, ldsv, lb, cbh, cbl, bhB, blB, acc2, accA, accB, bhB, blB, cj);
        stage<-1>(lds4, ldsv, lb, cbh, cbl, bhB, blB, acc2, accB, accA, bhA, blA, cj);
        stage<0>(lds4, ldsv, lb, cbh, cbl, bhA, blA, acc2, accA, accB, bhB, blB, cj);
        stage<1>(lds4, ldsv, lb, cbh, cbl, bhB, blB, acc2, accB, accA, bhA, blA, cj);
        stage<2>(lds4, ldsv, lb, cbh, cbl, bhA, blA, acc2, accA, accB, bhB, blB, cj);
        stage<3>(lds4, ldsv, lb, cbh, cbl, bhB, blB, acc2, accB, accA, bhA, blA, cj);
        stage<4>(lds4, ldsv, lb, cbh, cbl, bhA, blA, acc2, accA, accB, bhB, blB, cj);
        stage<5>(lds4, ldsv, lb, cbh, cbl, bhB, blB, acc2, accB, accA, bhA, blA, cj);
        tail(lds4, ldsv, lb, c2 * sc.r21, sc.S2, bhA, blA, acc2, acc3, cj);
        const size_t k = (size_t)t * n + e;
        float qv;
        if constexpr (QUANT) {
            qv = q_quantiles(lds, ldsv, lb, acc3, c3 * sc.r32, sc, lane, T.quantiles ? T.quantiles + k * (K_TAUS * A_OUT) : nullptr);
            if (T.taus && lane < 16) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) T.taus[k * K_TAUS + 16 * nt + col] = tau[nt];
            }
        } else {
            qv = q_mean(lds, ldsv, lb, acc3, c3 * sc.r32, sc, col);
        }
        float best = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qv), 0));
        int action = 0;
#define MN_ARG(a) { const float v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qv), a)); if (v > best) { best = v; action = a; } }
        MN_ARG(1) MN_ARG(2) MN_ARG(3) MN_ARG(4) MN_ARG(5) MN_ARG(6) MN_ARG(7) MN_ARG(8)
#undef MN_ARG
        if (T.q && lane < A_OUT) T.q[k * A_OUT + lane] = qv;
        if (T.cvar && lane == 0) T.cvar[k] = cv;
        __syncthreads();      // every lane has read the row before the step overwrites it
        // ---- step
        if constexpr (PARITY)
            if (T.traj) { A.traj = T.traj + (size_t)t * n * (size_t)P.N * 2; A.traj_n = P.N; }      // the step body records env e's N positions at [e][s] of this step's slice
        float *trow = T.obs ? T.obs + k * MN_OBS_DIM : nullptr;
        const MnStepOut o = ln.template step<false>(A, P, action, row, (PARITY && A.obs64) ? A.obs64 + (size_t)e * MN_OBS_DIM : nullptr, none,
                                                    nullptr, nullptr, trow);
        if (lane == 0) {
            if (T.reward) T.reward[k] = (float)o.reward;
            if (T.done) T.done[k] = (uint8_t)o.done;
            if (T.info) T.info[k] = (uint8_t)o.info;
            if (T.action) T.action[k] = action;
        }
        if (o.done) {      // (wave-uniform) terminal pose, counters and observation are final; the env idles for the rest of the launch
            last_info = o.info;
            steps = t + 1;
            break;
        }
    }
    ln.store(A);
    __syncthreads();
    for (int k = lane; k < MN_OBS_DIM; k += MN_WAVE) obs_io[(size_t)e * MN_OBS_DIM + k] = row[k];
    if (lane == 0)
        for (int t2 = steps; t2 < n_steps; ++t2) {
            const size_t k = (size_t)t2 * n + e;
            if (T.reward) T.reward[k] = 0.f;
            if (T.done) T.done[k] = 1;
            if (T.info) T.info[k] = (uint8_t)last_info;
            if (T.action) T.action[k] = -1;
        }
    // the act call counter: + the longest episode of the launch (GROUPED: of the group, in the group's own counter and words).  Every workgroup has read
    // counter0 before it takes its ticket, the last one writes (ticket words[0] and maximum words[1] are zero between launches).  Nobody waits for a ticket:
    // a grouped launch has far more workgroups than CUs, and a group's rows need not be resident together
    if (lane == 0) {
        __hip_atomic_fetch_max(words + 1, (uint32_t)steps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t old = __hip_atomic_fetch_add(words, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t last = GROUPED ? (uint32_t)G.rows - 1 : gridDim.x - 1;      // the ticket of the group's last arriver
        if (old == last) {
            const uint32_t s = __hip_atomic_load(words + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            rng_state[1] = ctr0 + s;
            if (steps_out) *steps_out = (int32_t)s;
            __hip_atomic_store(words + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(words, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace
