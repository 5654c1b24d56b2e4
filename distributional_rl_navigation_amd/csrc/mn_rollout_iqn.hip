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
// Floating-point contraction: the network is built like iqn_act.o (contraction allowed -- fast-honor-pragmas without a pragma compiles the
// per-row act kernels to the same code as -ffp-contract=fast), the step body and adjust_cvar under `#pragma clang fp contract(off)`, like
// the env kernels (mn_step.o / mn_rollout.o are built with -ffp-contract=off; the pragma reproduces that code object exactly).
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
};

constexpr int ROW_OFF = sp::ACT_IMG_FLOATS + F;                       // observation row, behind the acting image and the wave's feature buffer
constexpr int LDS_ROLL_FLOATS = ROW_OFF + 32;
static_assert(ROW_OFF % 4 == 0, "16-byte aligned row");

template <typename M, bool PARITY, int L>
__global__ __launch_bounds__(MN_WAVE, 1) void mn_rollout_iqn_kernel(MnArrays A, MnDev P, int n_steps, const uint32_t *__restrict__ packed,
                                                                    uint64_t *rng_state, float cvar, int adaptive, const float *__restrict__ cvar_row,
                                                                    const uint8_t *__restrict__ adaptive_row, float *__restrict__ obs_io, IqnTrace T,
                                                                    uint32_t *__restrict__ words, int32_t *__restrict__ steps_out) {
    using namespace sp;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using Lane = MnLane<M, PARITY, L>;
    const int lane = threadIdx.x, g = lane >> 4, col = lane & 15;
    const int e = blockIdx.x;
    const size_t n = (size_t)A.n;
    if (e == 0 && lane < 2 * MN_QSHARDS) A.queue_count[lane * MN_QSTRIDE] = 0u;   // nothing is left for a later mn_reset_done
    const uint64_t seed = rng_state[0], ctr0 = rng_state[1];
    // per-env cvar / adaptive flag (one env per wavefront: wave-uniform loads, outside the step loop); NULL = the launch's scalar
    if (cvar_row) cvar = cvar_row[e];
    if (adaptive_row) adaptive = adaptive_row[e];

    {   // the acting weight image (iqn_qvals_split_kernel's IMG for QUANT = false)
        const u32x4 *src = reinterpret_cast<const u32x4 *>(packed);
        u32x4 *dst = reinterpret_cast<u32x4 *>(lds);
        for (int i = lane; i < OFF_W4H / 4; i += MN_WAVE) dst[i] = src[i];
    }
    float *row = lds + ROW_OFF;
    for (int k = lane; k < MN_OBS_DIM; k += MN_WAVE) row[k] = obs_io[(size_t)e * MN_OBS_DIM + k];     // the observation the episode continues from

    const f32x4 *ldsv = reinterpret_cast<const f32x4 *>(lds);
    const u32x4 *lds4 = reinterpret_cast<const u32x4 *>(lds);
    LdsBase lb;
    lb.w_lo = lane; lb.w_hi = lane + 4096; lb.fl = (OFF_B1 >> 2) + g; lb.fb = (OFF_W4H >> 2) + g;
    int enc_w = (OFF_WS >> 2) + lane, enc_f = OFF_BND + lane, fb_f = OFF_W4H + lane;
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
        const float cv = adaptive ? adjust_cvar_row(row) : cvar;
        uint32_t k0, k1;
        draw_keys(seed, ctr0 + (uint64_t)t, k0, k1);
        float tau[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) tau[nt] = tau_draw(e, 16 * nt + col, k0, k1, cv);
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
        for (int i = 0; i < 28; ++i) ov[i] = i < OBS ? row[i] : 0.f;
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
        const float qv = q_mean(lds, ldsv, lb, acc3, c3 * sc.r32, sc, col);
        float best = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qv), 0));
        int action = 0;
#define MN_ARG(a) { const float v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qv), a)); if (v > best) { best = v; action = a; } }
        MN_ARG(1) MN_ARG(2) MN_ARG(3) MN_ARG(4) MN_ARG(5) MN_ARG(6) MN_ARG(7) MN_ARG(8)
#undef MN_ARG
        const size_t k = (size_t)t * n + e;
        if (T.q && lane < A_OUT) T.q[k * A_OUT + lane] = qv;
        if (T.cvar && lane == 0) T.cvar[k] = cv;
        __syncthreads();      // every lane has read the row before the step overwrites it
        // ---- step
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
    // the act call counter: + the longest episode of the launch.  Every workgroup has read counter0 before it takes its ticket, the last one
    // writes (ticket words[0] and maximum words[1] are zero between launches)
    if (lane == 0) {
        __hip_atomic_fetch_max(words + 1, (uint32_t)steps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t old = __hip_atomic_fetch_add(words, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old == gridDim.x - 1) {
            const uint32_t s = __hip_atomic_load(words + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            rng_state[1] = ctr0 + s;
            if (steps_out) *steps_out = (int32_t)s;
            __hip_atomic_store(words + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(words, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

void mn_launch_rollout_iqn_rows(const MnArrays &A, const MnDev &P, int precision, int n_steps, const uint32_t *image, uint64_t *rng_state, float cvar,
                                int adaptive, const float *cvar_row, const uint8_t *adaptive_row, float *obs_io, float *obs_trace, float *reward_trace,
                                uint8_t *done_trace, uint8_t *info_trace, int32_t *action_trace, float *cvar_trace, float *q_trace, uint32_t *words,
                                int32_t *steps_run, hipStream_t s) {
    const IqnTrace T = {obs_trace, reward_trace, done_trace, info_trace, action_trace, cvar_trace, q_trace};
    constexpr int LL = 8;      // the lane groups of mn_rollout_policy_kernel
    const size_t lds_bytes = LDS_ROLL_FLOATS * sizeof(float);
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
