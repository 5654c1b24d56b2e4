// mn_rollout_dqn.hip -- DQN evaluation episodes in ONE launch (gfx950): mn_rollout_policy's episode semantics with the DQN baseline's greedy policy.
//
// train_dqn.evaluate and the DQN rows of experiments.run_experiment run one Python iteration per env step (mn_dqn_act, mn_step, half a dozen small
// torch kernels).  Here a wavefront owns EIGHT environments for the whole launch (8 lanes per env, the lane groups of mn_rollout_policy_kernel) and,
// per step, runs the seven dense<> stages of dqn_qvals_kernel (dqn_net.h: same device functions, same LDS image, same k order) with its
// environments in MFMA columns 0-7 -- columns 8-15 read zero rows --, the first-maximum argmax, then the same MnLane::step as everywhere else.  An
// MFMA column depends on its own environment only, so the result is bit-identical to a loop of (mn_dqn_act, mn_step) on the same state.
//
// One wavefront per workgroup (the step's sonar work-list is workgroup LDS); the weight image (IMAGE_FLOATS, packed by dqn_pack_kernel) is dynamic
// LDS and fills most of a CU's 160 KB, so a workgroup has its CU to itself: 30 evaluation worlds are 4 CUs, 500 sweep worlds 63.
//
// Built like mn_rollout.o (-ffp-contract=off -fno-slp-vectorize, which the step body needs): the network is MFMA and fmaxf only, nothing in it contracts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mn_step_body.h"

namespace {

#include "dqn_net.h"

struct DqnTrace {
    float *obs;        // [T][n][26] observation each step returned (not written once the env has finished)
    float *reward;     // [T][n]     0 once finished
    uint8_t *done;     // [T][n]     1 once finished
    uint8_t *info;     // [T][n]     the terminal code once finished
    int32_t *action;   // [T][n]     -1 once finished
    float *q;          // [T][n][9]  Q(s, .) the action was chosen from (not written once finished)
    double *traj;      // [T][n][N][2] the step's sub-step positions (mn_set_trajectory_trace; float64 handles; not written once finished)
};

template <typename M, bool PARITY, int L>
__global__ __launch_bounds__(MN_WAVE, 1) void mn_rollout_dqn_kernel(MnArrays A, MnDev P, int n_steps, const float *__restrict__ image, float *__restrict__ obs_io,
                                                                    DqnTrace T) {
    static_assert(L == 8, "eight envs per wavefront sit in MFMA columns 0-7");
    constexpr int EPW = MN_WAVE / L;                                     // envs per wavefront
    extern __shared__ __attribute__((aligned(16))) float lds[];          // the weight image
    __shared__ __attribute__((aligned(16))) float rows[16][32];          // observation rows of the wave's envs, zero-padded; rows 8-15 stay zero
    using Lane = MnLane<M, PARITY, L>;
    const int lane = threadIdx.x, g = lane >> 4, col = lane & 15;
    const int tid = blockIdx.x * MN_WAVE + lane;
    const int e = tid / L, q = tid % L, slot = lane / L;
    const size_t n = (size_t)A.n;
    if (tid < 2 * MN_QSHARDS) A.queue_count[tid * MN_QSTRIDE] = 0u;      // nothing is left for a later mn_reset_done
    {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(image);
        f32x4 *dst = reinterpret_cast<f32x4 *>(lds);
        for (int i = lane; i < IMAGE_FLOATS / 4; i += MN_WAVE) dst[i] = src[i];
    }
    const MnRing none = {};
    Lane ln;
    ln.load(A, e, q);
    for (int k = lane; k < 16 * 32; k += MN_WAVE) rows[k >> 5][k & 31] = 0.f;
    __syncthreads();
    // the observation the episode continues from (mn_reset / mn_load_worlds left it in obs_io)
    if (ln.active)
        for (int k = q; k < MN_OBS_DIM; k += L) rows[slot][k] = obs_io[(size_t)e * MN_OBS_DIM + k];
    bool alive = ln.active;
    int last_info = 0;
    const int e_col = blockIdx.x * EPW + col;                            // the env in this lane's MFMA column (col < 8)
    for (int t = 0; t < n_steps; ++t) {
        __syncthreads();      // (one wavefront per workgroup) the rows of the previous step are complete
        // ---- act: dqn_qvals_kernel's forward pass and argmax on the float32 rows
        f32x4 x0[2];
        x0[0] = *reinterpret_cast<const f32x4 *>(&rows[col][4 * g]);
        x0[1] = *reinterpret_cast<const f32x4 *>(&rows[col][16 + 4 * g]);
        const f32x4 qv = dqn_forward(lds, lane, x0);
        const int arg = dqn_argmax(qv, g);
        const unsigned long long alive_mask = __ballot(alive);
        if (T.q && col < EPW && ((alive_mask >> (L * col)) & 1ull)) {
            float *qrow = T.q + ((size_t)t * n + e_col) * MN_NUM_ACTIONS;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * g + r < MN_NUM_ACTIONS) qrow[4 * g + r] = qv[r];
        }
        int action = __shfl(arg, slot);      // lane (g = 0, col = slot) holds the action of this lane group's env
        if (!alive) action = 0;
        __syncthreads();      // every lane has read the rows before the step overwrites them
        // ---- step
        float *trow = T.obs ? T.obs + ((size_t)t * n + (ln.active ? e : 0)) * MN_OBS_DIM : nullptr;
        if constexpr (PARITY)      // the step body records env e's N sub-step positions at [e][s] of this step's slice while the env is alive
            if (T.traj) { A.traj = alive ? T.traj + (size_t)t * n * (size_t)P.N * 2 : nullptr; A.traj_n = P.N; }
        const MnStepOut o = ln.template step<false>(A, P, action, rows[slot], (PARITY && A.obs64 && alive) ? A.obs64 + (size_t)e * MN_OBS_DIM : nullptr, none,
                                                    nullptr, nullptr, (alive && trow) ? trow : nullptr);
        if (ln.active && q == 0) {
            const size_t k = (size_t)t * n + e;
            if (T.reward) T.reward[k] = alive ? (float)o.reward : 0.f;
            if (T.done) T.done[k] = alive ? (uint8_t)o.done : (uint8_t)1;
            if (T.info) T.info[k] = alive ? (uint8_t)o.info : (uint8_t)last_info;
            if (T.action) T.action[k] = alive ? action : -1;
        }
        if (alive && o.done) {      // terminal pose, counters and observation of this env are final
            ln.store(A);
            __builtin_amdgcn_wave_barrier();
            for (int k = q; k < MN_OBS_DIM; k += L) obs_io[(size_t)e * MN_OBS_DIM + k] = rows[slot][k];
            last_info = o.info;
            alive = false;
        }
        // (an env that has finished keeps stepping from its terminal pose -- the lane group's cross-lane work is wave-uniform -- but nothing of it is
        // stored or traced, incl. the float64 copies of mn_enable_obs64; its column of the next forward pass is computed and dropped)
        if (!__any(alive)) {      // the whole wave is done: fill the remaining trace entries and leave
            for (int t2 = t + 1; t2 < n_steps; ++t2)
                if (ln.active && q == 0) {
                    const size_t k = (size_t)t2 * n + e;
                    if (T.reward) T.reward[k] = 0.f;
                    if (T.done) T.done[k] = 1;
                    if (T.info) T.info[k] = (uint8_t)last_info;
                    if (T.action) T.action[k] = -1;
                }
            return;
        }
    }
    if (alive) {      // still running after n_steps: the state the next call continues from
        ln.store(A);
        __builtin_amdgcn_wave_barrier();
        for (int k = q; k < MN_OBS_DIM; k += L) obs_io[(size_t)e * MN_OBS_DIM + k] = rows[slot][k];
    }
}

}  // namespace

void mn_launch_rollout_dqn(const MnArrays &A, const MnDev &P, int precision, int n_steps, const float *image, float *obs_io, float *obs_trace,
                           float *reward_trace, uint8_t *done_trace, uint8_t *info_trace, int32_t *action_trace, float *q_trace, double *traj_trace, hipStream_t s) {
    const DqnTrace T = {obs_trace, reward_trace, done_trace, info_trace, action_trace, q_trace, traj_trace};
    constexpr int LL = 8;
    const dim3 grid((unsigned)((A.n + MN_WAVE / LL - 1) / (MN_WAVE / LL)));      // (npad is a multiple of 256: the last wave's idle lane groups load padding)
    const size_t lds_bytes = IMAGE_FLOATS * sizeof(float);
    if (precision == MN_PRECISION_F64) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_rollout_dqn_kernel<double, true, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL((mn_rollout_dqn_kernel<double, true, LL>), grid, dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, image, obs_io, T);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mn_rollout_dqn_kernel<float, false, LL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        hipLaunchKernelGGL((mn_rollout_dqn_kernel<float, false, LL>), grid, dim3(MN_WAVE), lds_bytes, s, A, P, n_steps, image, obs_io, T);
    }
}
