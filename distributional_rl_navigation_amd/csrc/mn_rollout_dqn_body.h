// mn_rollout_dqn_body.h -- DQN evaluation episodes, eight environments per wavefront: the body of the DQN episode launches.
// Included ONCE by mn_rollout_dqn.hip (GROUPED = false: one weight image for the whole launch, mn_rollout_dqn) and by mn_rollout_dqn_groups.hip
// (GROUPED = true: every group of rows its own weight image, mn_rollout_dqn_groups); each wraps dqn_episode<> in its own __global__ kernel.  Both files
// are built like mn_rollout.o (-ffp-contract=off -fno-slp-vectorize, which the step body needs): the network is MFMA and fmaxf only, nothing in it contracts.
//
// A wavefront owns EIGHT environments for the whole launch (8 lanes per env, the lane groups of mn_rollout_policy_kernel) and, per step, runs the seven
// dense<> stages of dqn_qvals_kernel (dqn_net.h: same device functions, same LDS image, same k order) with its environments in MFMA columns 0-7 --
// columns 8-15 read zero rows --, the first-maximum argmax, then the same MnLane::step as everywhere else.  An MFMA column depends on its own
// environment only, so the result is bit-identical to a loop of (mn_dqn_act, mn_step) on the same state.
//
// One wavefront per workgroup (the step's sonar work-list is workgroup LDS); the weight image (IMAGE_FLOATS, packed by dqn_pack_kernel) is dynamic
// LDS and fills most of a CU's 160 KB, so a workgroup has its CU to itself.
#pragma once
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

// Which rows of a launch act together (GROUPED = true): row e of the handle belongs to group e / rows and is row e % rows of it.  A group has its own
// weight image (image + group * stride) and `wpg` = ceil(rows / 8) wavefronts (= workgroups) of its own: workgroup w serves group w / wpg as its
// local wave w % wpg, whose lane group `slot` holds the group's row 8 * (w % wpg) + slot.  rows need not be a multiple of 8: the slots of the last local
// wave behind the group's last row are PADDING -- they would otherwise address the first rows of the next group.  A padding slot is never active and
// never alive: it loads the group's last row (in bounds, whatever the group), stores nothing -- pose, counters, obs_io, traces, Q trace -- and its
// column of the forward pass is computed and dropped, as a finished env's.
// GROUPED = false: one group, the whole launch -- the descriptor is not read, and the idle lane groups of the last wave are the rows n .. npad.
struct DqnGroups {
    int rows;          // rows per group
    int wpg;           // wavefronts (workgroups) per group: ceil(rows / 8)
    int64_t stride;    // floats from one group's weight image to the next (a multiple of 4: the image is staged 16 bytes at a time)
};

// NOISE (mn_set_obs_noise): the network reads what the robot perceives -- a second set of rows in LDS, filled at the head of a step by each lane group from
// its clean row under the key (seed, global env index, the lane's ep_t) -- while the step keeps writing the clean rows: obs_io and the traces are what they
// are without noise.  NOISE = false is the body as it was; `NS` is not read.
template <typename M, bool PARITY, int L, bool GROUPED, bool NOISE = false>
__device__ __forceinline__ void dqn_episode(float *lds, MnArrays A, const MnDev &P, int n_steps, const float *__restrict__ image, float *__restrict__ obs_io,
                                            const DqnTrace &T, const DqnGroups &G, const MnObsNoiseArg &NS = MnObsNoiseArg{}) {
    static_assert(L == 8, "eight envs per wavefront sit in MFMA columns 0-7");
    constexpr int EPW = MN_WAVE / L;                                     // envs per wavefront
    __shared__ __attribute__((aligned(16))) float rows[16][32];          // observation rows of the wave's envs, zero-padded; rows 8-15 stay zero
    __shared__ __attribute__((aligned(16))) float seen[NOISE ? 16 : 1][NOISE ? 32 : 4];      // NOISE: the perceived rows, zero-padded like `rows`
    using Lane = MnLane<M, PARITY, L>;
    const int lane = threadIdx.x, g = lane >> 4, col = lane & 15;
    const int tid = blockIdx.x * MN_WAVE + lane;
    const int q = tid % L, slot = lane / L;
    const size_t n = (size_t)A.n;
    if (tid < 2 * MN_QSHARDS) A.queue_count[tid * MN_QSTRIDE] = 0u;      // nothing is left for a later mn_reset_done
    // e: the env of this lane's lane group; e_col: the env in this lane's MFMA column (col < 8); *_real: a row of the launch, not padding
    int e, e_col;
    bool real = true, col_real = true;
    if constexpr (GROUPED) {
        const int grp = blockIdx.x / G.wpg, r0 = (blockIdx.x - grp * G.wpg) * EPW, base = grp * G.rows;
        real = r0 + slot < G.rows;
        col_real = r0 + col < G.rows;
        e = base + min(r0 + slot, G.rows - 1);
        e_col = base + min(r0 + col, G.rows - 1);
        image += (size_t)grp * (size_t)G.stride;
    } else {
        e = tid / L;
        e_col = blockIdx.x * EPW + col;
    }
    {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(image);
        f32x4 *dst = reinterpret_cast<f32x4 *>(lds);
        for (int i = lane; i < IMAGE_FLOATS / 4; i += MN_WAVE) dst[i] = src[i];
    }
    const MnRing none = {};
    Lane ln;
    ln.load(A, e, q);
    if constexpr (GROUPED) ln.active = ln.active && real;
    for (int k = lane; k < 16 * 32; k += MN_WAVE) rows[k >> 5][k & 31] = 0.f;
    if constexpr (NOISE)
        for (int k = lane; k < 16 * 32; k += MN_WAVE) seen[k >> 5][k & 31] = 0.f;
    __syncthreads();
    // the observation the episode continues from (mn_reset / mn_load_worlds left it in obs_io)
    if (ln.active)
        for (int k = q; k < MN_OBS_DIM; k += L) rows[slot][k] = obs_io[(size_t)e * MN_OBS_DIM + k];
    bool alive = ln.active;
    int last_info = 0;
    for (int t = 0; t < n_steps; ++t) {
        __syncthreads();      // (one wavefront per workgroup) the rows of the previous step are complete
        // ---- act: dqn_qvals_kernel's forward pass and argmax on the float32 rows
        f32x4 x0[2];
        if constexpr (NOISE) {
            const uint64_t key = mn_obs_noise_row_key(NS.S.seed, NS.env0 + (uint64_t)e, (uint64_t)(int64_t)ln.ep_t);
            for (int c = q; c < MN_OBS_NOISE_CHANNELS; c += L) mn_obs_noise_channel(rows[slot], seen[slot], c, key, NS.S);
            __syncthreads();      // the perceived rows are complete
            x0[0] = *reinterpret_cast<const f32x4 *>(&seen[col][4 * g]);
            x0[1] = *reinterpret_cast<const f32x4 *>(&seen[col][16 + 4 * g]);
        } else {
            x0[0] = *reinterpret_cast<const f32x4 *>(&rows[col][4 * g]);
            x0[1] = *reinterpret_cast<const f32x4 *>(&rows[col][16 + 4 * g]);
        }
        const f32x4 qv = dqn_forward(lds, lane, x0);
        const int arg = dqn_argmax(qv, g);
        const unsigned long long alive_mask = __ballot(alive);
        if (T.q && col < EPW && col_real && ((alive_mask >> (L * col)) & 1ull)) {
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
