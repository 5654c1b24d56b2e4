// mn_query_step.hip -- mn_query_rollout (gfx950): what-if steps and open-loop rollouts of robots the caller places by hand, in
// worlds the handle holds, without stepping anything the handle owns (arithmetic: mn_query_step_body.h on mn_query_body.h).
//
// Mapping: mn_query.hip's.  One lane per query, 256-lane workgroups, a grid-stride loop over the queries; a query is independent
// of every other one: no LDS, no atomics, no cross-lane traffic, no RNG, no policy (closed-loop episodes are the episode kernels').
//   * UNIFORM (env_of_query == NULL): the world's index is a kernel argument, its cores are read once per wavefront in front of
//     the loop (scalar loads) and the obstacle passes walk one address per wavefront.
//   * per-query worlds: lane q gathers rows [k][env] of the SoA tables for its own env -- the cores at every sub-step (they are not held
//     in vector registers over the rollout; the reads hit the cache) --; an index outside [0, n) reads nothing.
// Lane q runs its steps one after the other and stops at `done` (or at its own length); the lanes of a wavefront that are finished
// wait for the longest one, as in every one-lane-per-item loop.  The sonar runs ONCE per query, on the state the query ends in
// (no trace holds observations); the steps in between form only the flag bits (mnq_flags).
// The kernels only READ the handle's master tables; their stores go to the caller's output buffers alone.
#include "mn_query_step_body.h"

#define MNQ_BLOCK 256
#define MNQ_MAX_BLOCKS 2048

struct MnqRolloutArgs {
    const int32_t *env_of;
    int env0;
    const double *state;          // [Q][6]
    const int32_t *ep_t;          // [Q] or NULL = 0
    int action_mode;
    const int32_t *actions;       // [H] | [Q] | [Q][H]
    int n_steps;                  // H
    const int32_t *n_steps_of;    // [Q] or NULL = H
    long long nq;
    double *state_out;            // [Q][6]
    float *obs;                   // [Q][26]
    double *obs64;                // [Q][26]
    double *reward;               // [Q]
    uint8_t *done, *info;         // [Q]
    int32_t *steps;               // [Q]
    double *reward_tr;            // [H][Q]
    uint8_t *done_tr, *info_tr;   // [H][Q]
    int32_t *action_tr;           // [H][Q]
    double *state_tr;             // [H][Q][6]
    double *traj_tr;              // [H][Q][N][2]
};

// (mnqs_load_cores, MnqsObstacles and MnqsRowOut are the twins of mn_query.hip's table readers and row sink, which live in that translation unit)
__device__ __forceinline__ void mnqs_load_cores(const MnArrays &A, int e, MnqCores &W) {
    const int np = A.npad;
    W.nc = A.counts[e] & 0xff;
#pragma unroll
    for (int k = 0; k < MN_MAX_CORES; ++k) {
        W.cx[k] = A.cx[(size_t)k * np + e]; W.cy[k] = A.cy[(size_t)k * np + e]; W.cg[k] = A.cg[(size_t)k * np + e];
    }
}

// the cores of a step: held in front of the query loop (UNIFORM: scalar registers), or read from the tables at every sub-step (a world per lane: 24
// loads that hit the cache against 48 vector registers held over the whole rollout, which the kernel does not have)
template <bool HELD>
struct MnqsCores {
    const MnArrays &A;
    const MnqCores &held;
    int e;
    __device__ __forceinline__ void cores(MnqCores &W) const {
        if (HELD) { W = held; return; }
        int ee = e;
        asm volatile("" : "+v"(ee));      // a fresh read per sub-step: nothing to keep live between them
        mnqs_load_cores(A, ee, W);
    }
};

struct MnqsObstacles {
    const double *__restrict__ ox, *__restrict__ oy, *__restrict__ orad;
    int np, e;
    __device__ __forceinline__ void obstacle(int k, double &x, double &y, double &r) const {
        const size_t at = (size_t)k * np + e;
        x = ox[at]; y = oy[at]; r = orad[at];
    }
};

struct MnqsRowOut {
    float *o32;
    double *o64;
    __device__ __forceinline__ void pair(int at, double a, double b) {
        if (o32) *reinterpret_cast<float2 *>(o32 + at) = make_float2((float)a, (float)b);
        if (o64) { o64[at] = a; o64[at + 1] = b; }
    }
    __device__ __forceinline__ void head(double o0, double o1, double o2, double o3) { pair(0, o0, o1); pair(2, o2, o3); }
    __device__ __forceinline__ void beam(int i, double bx, double by) { pair(4 + 2 * i, bx, by); }
};

// the sub-step positions of one step of one query, or nowhere
struct MnqsTraj {
    double *p;
    __device__ __forceinline__ void point(int i, double x, double y) {
        if (p) { p[2 * i] = x; p[2 * i + 1] = y; }
    }
};

template <bool UNIFORM>
__global__ __launch_bounds__(MNQ_BLOCK) void mn_query_rollout_kernel(const MnArrays A, const MnDev P, const MnqRolloutArgs R) {
    MnqCores W = {};
    if (UNIFORM) mnqs_load_cores(A, R.env0, W);
    const double nan = __builtin_nan("");
    const bool traced = R.reward_tr || R.done_tr || R.info_tr || R.action_tr || R.state_tr || R.traj_tr;
    const long long nq = R.nq;
    const long long stride = (long long)gridDim.x * MNQ_BLOCK;
    for (long long q = (long long)blockIdx.x * MNQ_BLOCK + threadIdx.x; q < nq; q += stride) {
        const int e = UNIFORM ? R.env0 : R.env_of[q];
        const bool bad_env = !UNIFORM && (e < 0 || e >= A.n);
        int n_q = R.n_steps_of ? R.n_steps_of[q] : R.n_steps;
        n_q = n_q < 0 ? 0 : (n_q > R.n_steps ? R.n_steps : n_q);
        const double *st = R.state + q * 6;
        MnqRobot r = {st[0], st[1], st[2], st[3], st[4], st[5]};
        const int ep0 = R.ep_t ? R.ep_t[q] : 0;
        double reward = 0.0, gx = 0.0, gy = 0.0;
        int info = MN_INFO_NORMAL, steps = 0, no = 0;
        bool done = false, poisoned = false;
        const MnqsObstacles obst = {A.ox, A.oy, A.orad, A.npad, bad_env ? 0 : e};
        const MnqsCores<UNIFORM> cores = {A, W, obst.e};
        if (bad_env) {      // finished before it began: no table is read
            poisoned = true; done = true; info = MN_QUERY_FLAG_BAD_ENV; reward = nan;
        } else {
            no = (A.counts[e] >> 8) & 0xff;
            gx = A.goal_x[e]; gy = A.goal_y[e];
        }
        for (int t = 0; t < R.n_steps; ++t) {
            const bool live = !done && t < n_q;
            if (!live && !traced) break;
            const size_t row = (size_t)t * (size_t)nq + (size_t)q;
            MnqsTraj traj = {R.traj_tr ? R.traj_tr + row * (size_t)P.N * 2 : nullptr};
            int act = -1;
            bool moved = false;
            if (live) {
                act = R.action_mode == MN_QUERY_ACTIONS_SHARED ? R.actions[t]
                      : (R.action_mode == MN_QUERY_ACTIONS_CONSTANT ? R.actions[q] : R.actions[(size_t)q * (size_t)R.n_steps + t]);
                if (!mnq_state_ok(r) || act < 0 || act >= MN_NUM_ACTIONS) {
                    poisoned = true; done = true; info = MN_QUERY_INFO_BAD_STATE; reward = nan;
                } else {
                    info = mnq_step(cores, obst, no, gx, gy, P, act, ep0 + t, r, reward, traj);
                    done = info != MN_INFO_NORMAL;
                    moved = true;
                }
                steps = t + 1;
            }
            if (poisoned) { r.x = nan; r.y = nan; r.theta = nan; r.speed = nan; r.vx = nan; r.vy = nan; }
            if (R.reward_tr) R.reward_tr[row] = live ? reward : 0.0;
            if (R.done_tr) R.done_tr[row] = live ? (uint8_t)done : (uint8_t)1;
            if (R.info_tr) R.info_tr[row] = (uint8_t)info;
            if (R.action_tr) R.action_tr[row] = act;
            if (R.state_tr) {
                double *o = R.state_tr + row * 6;
                o[0] = r.x; o[1] = r.y; o[2] = r.theta; o[3] = r.speed; o[4] = r.vx; o[5] = r.vy;
            }
            if (traj.p && !moved)
                for (int i = 0; i < P.N; ++i) traj.point(i, nan, nan);
        }
        if (poisoned) { r.x = nan; r.y = nan; r.theta = nan; r.speed = nan; r.vx = nan; r.vy = nan; }
        if (R.state_out) {
            double *o = R.state_out + q * 6;
            o[0] = r.x; o[1] = r.y; o[2] = r.theta; o[3] = r.speed; o[4] = r.vx; o[5] = r.vy;
        }
        if (R.obs || R.obs64) {
            MnqsRowOut out;
            out.o32 = R.obs ? R.obs + q * MN_OBS_DIM : nullptr;
            out.o64 = R.obs64 ? R.obs64 + q * MN_OBS_DIM : nullptr;
            if (poisoned) {
                for (int i = 0; i < MN_OBS_DIM; i += 2) out.pair(i, nan, nan);
            } else {
                mnq_observe(obst, no, gx, gy, P, r.x, r.y, r.theta, r.vx, r.vy, out);
            }
        }
        if (R.reward) R.reward[q] = reward;
        if (R.done) R.done[q] = (uint8_t)done;
        if (R.info) R.info[q] = (uint8_t)info;
        if (R.steps) R.steps[q] = steps;
    }
}

void mn_launch_query_rollout(const MnArrays &A, const MnDev &P, const int32_t *env_of, int env0, const double *state, const int32_t *ep_t, int action_mode,
                             const int32_t *actions, int n_steps, const int32_t *n_steps_of, int64_t nq, double *state_out, float *obs, double *obs64,
                             double *reward, uint8_t *done, uint8_t *info, int32_t *steps, double *reward_tr, uint8_t *done_tr, uint8_t *info_tr,
                             int32_t *action_tr, double *state_tr, double *traj_tr, hipStream_t s) {
    const MnqRolloutArgs R = {env_of, env0, state, ep_t, action_mode, actions, n_steps, n_steps_of, (long long)nq, state_out, obs, obs64, reward, done, info,
                              steps, reward_tr, done_tr, info_tr, action_tr, state_tr, traj_tr};
    const int64_t b = (nq + MNQ_BLOCK - 1) / MNQ_BLOCK;
    const dim3 grid((unsigned)(b < MNQ_MAX_BLOCKS ? b : MNQ_MAX_BLOCKS)), block(MNQ_BLOCK);
    if (env_of) hipLaunchKernelGGL(mn_query_rollout_kernel<false>, grid, block, 0, s, A, P, R);
    else hipLaunchKernelGGL(mn_query_rollout_kernel<true>, grid, block, 0, s, A, P, R);
}
