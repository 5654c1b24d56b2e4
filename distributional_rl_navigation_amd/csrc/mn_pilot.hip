// mn_pilot.hip -- the field pilot (gfx950): mn_pilot_act, the pilot's action for robots the caller places by hand, and mn_rollout_pilot, whole
// episodes of the handle's envs under the pilot in one launch (rule and arithmetic: mn_pilot_body.h on mn_query_step_body.h; the real step:
// mn_step_body.h).
//
// Mapping, both kernels: a ROW of 16 lanes (one DPP row) serves one robot, a wavefront holds four.  Lanes 0-8 of the row run the nine candidates
// side by side -- lane a holds action a: a copy of the state, up to H what-if steps, the landing point's interpolated field value --, lanes 9-15
// idle through that phase.  The key (score, H - n, a) is reduced over the row by four DPP stages (quad_perm, quad_perm, row_half_mirror,
// row_mirror: no LDS, every lane ends with the row's least key).  A candidate reads its world from the float64 master tables lane by lane (the
// cores at every sub-step: the reads hit the cache; nothing is held over the rollout) and the field from global memory (five words per candidate).
//   mn_pilot_act:      256-lane workgroups, a grid-stride loop over groups of 16 queries; lanes 0-8 store their own score / steps / info, lane 0
//                      the action and the flag byte.  Reads the handle's tables only.
//   mn_rollout_pilot:  one wavefront per workgroup, four envs per wavefront (MnLane<double, true, 16>).  Per step: the candidates from the env's own
//                      float64 pose and counter as the registers hold them -- the words mn_get_state would return --, the row's choice, then
//                      MnLane::step on the same 16 lanes.  So the launch is bit for bit the loop (mn_get_state, mn_pilot_act, mn_step).  An env
//                      that has finished idles (its lanes keep running the wave-uniform step with every store switched off).
#include "mn_pilot_body.h"
#include "mn_step_body.h"

#define MNP_ROW 16
#define MNP_BLOCK 256

namespace {

struct MnpCores {      // the cores of world e, read from the tables at every sub-step (mn_query_step.hip's per-lane form)
    const MnArrays &A;
    int e;
    __device__ __forceinline__ void cores(MnqCores &W) const {
        int ee = e;
        asm volatile("" : "+v"(ee));      // a fresh read per sub-step: nothing to keep live between them
        const int np = A.npad;
        W.nc = A.counts[ee] & 0xff;
#pragma unroll
        for (int k = 0; k < MN_MAX_CORES; ++k) {
            W.cx[k] = A.cx[(size_t)k * np + ee]; W.cy[k] = A.cy[(size_t)k * np + ee]; W.cg[k] = A.cg[(size_t)k * np + ee];
        }
    }
};

struct MnpObstacles {
    const double *__restrict__ ox, *__restrict__ oy, *__restrict__ orad;
    int np, e;
    __device__ __forceinline__ void obstacle(int k, double &x, double &y, double &r) const {
        const size_t at = (size_t)k * np + e;
        x = ox[at]; y = oy[at]; r = orad[at];
    }
};

struct MnpField {
    const double *__restrict__ T_;
    __device__ __forceinline__ double T(int c) const { return T_[c]; }
};

// one stage of the row's key reduction: take the partner's key if it is the lesser one
template <int CTRL>
__device__ __forceinline__ void mnp_key_step(double &score, int &rem, int &a) {
    const double os = dpp_get<CTRL>(score);
    const int orem = __builtin_amdgcn_update_dpp(0, rem, CTRL, 0xF, 0xF, true);
    const int oa = __builtin_amdgcn_update_dpp(0, a, CTRL, 0xF, 0xF, true);
    const bool take = mnp_better(os, orem, oa, score, rem, a);
    score = take ? os : score; rem = take ? orem : rem; a = take ? oa : a;
}
// the least key of the 16 lanes of a row, in every lane of it (keys are distinct in `a`, so every lane settles on the same one)
__device__ __forceinline__ void mnp_row_best(double &score, int &rem, int &a) {
    mnp_key_step<0xB1>(score, rem, a);       // quad_perm [1,0,3,2]
    mnp_key_step<0x4E>(score, rem, a);       // quad_perm [2,3,0,1]
    mnp_key_step<0x141>(score, rem, a);      // row_half_mirror
    mnp_key_step<0x140>(score, rem, a);      // row_mirror
}

// The nine candidates of one robot over its row and the row's choice.  `ok`: the robot is to be served (row-uniform); q: the lane within the row.
// Lane q < 9 leaves with its own score / n / info, every lane with the chosen action.
__device__ __forceinline__ int mnp_row_act(const MnArrays &A, const MnDev &P, bool ok, int q, int e, const double *Tf, int nx, int ny, int H,
                                           const MnqRobot &r0, int t, double &score, int &n, int &info) {
    score = (double)INFINITY; n = 0; info = MN_INFO_NORMAL;
    int rem = H + 1, a = q;      // (lanes 9-15: a key behind every candidate's)
    if (ok && q < MN_NUM_ACTIONS) {
        const MnpObstacles obst = {A.ox, A.oy, A.orad, A.npad, e};
        const MnpCores cores = {A, e};
        const MnpField F = {Tf};
        const int no = (A.counts[e] >> 8) & 0xff;
        MnqRobot r = r0;
        score = mnp_candidate(cores, obst, no, A.goal_x[e], A.goal_y[e], P, F, nx, ny, H, q, t, r, n, info);
        rem = H - n;
    }
    double bs = score;
    mnp_row_best(bs, rem, a);
    return a;
}

struct MnpActArgs {
    const int32_t *env_of;
    int env0;
    const double *state;          // [Q][6]
    const int32_t *ep_t;          // [Q] or NULL = 0
    const double *T;              // [n_fields][ny][nx]
    const int32_t *field_of;      // [Q] or NULL = field 0
    long long n_fields;
    int nx, ny, H;
    long long nq;
    int32_t *actions;             // [Q]
    double *scores;               // [Q][9]
    int32_t *steps;               // [Q][9]
    uint8_t *infos;               // [Q][9]
    uint8_t *flags;               // [Q]
};

__global__ __launch_bounds__(MNP_BLOCK) void mn_pilot_act_kernel(const MnArrays A, const MnDev P, const MnpActArgs R) {
    const int q = threadIdx.x & (MNP_ROW - 1);
    const long long rows_per_block = MNP_BLOCK / MNP_ROW;
    const long long n_groups = (R.nq + rows_per_block - 1) / rows_per_block;
    const size_t nc = (size_t)R.nx * R.ny;
    // (the loop bound is workgroup-uniform, and a row past the last query runs along unserved: the DPP stages see whole rows)
    for (long long g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const long long i = g * rows_per_block + threadIdx.x / MNP_ROW;
        const bool there = i < R.nq;
        int e = 0, flag = 0, t = 0;
        long long f = 0;
        MnqRobot r = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (there) {
            e = R.env_of ? R.env_of[i] : R.env0;
            f = R.field_of ? (long long)R.field_of[i] : 0;
            const double *st = R.state + i * 6;
            r = {st[0], st[1], st[2], st[3], st[4], st[5]};
            t = R.ep_t ? R.ep_t[i] : 0;
            if (e < 0 || e >= A.n) flag = MN_QUERY_FLAG_BAD_ENV;
            else if (f < 0 || f >= R.n_fields) flag = MN_PILOT_FLAG_BAD_FIELD;
            else if (!mnq_state_ok(r)) flag = MN_QUERY_INFO_BAD_STATE;
            else { const double t0 = R.T[(size_t)f * nc]; if (t0 != t0) flag = MN_PILOT_FLAG_BAD_FIELD; }
        }
        const bool ok = there && flag == 0;
        double score;
        int n, info;
        const int action = mnp_row_act(A, P, ok, q, ok ? e : 0, R.T + (ok ? (size_t)f * nc : 0), R.nx, R.ny, R.H, r, t, score, n, info);
        if (there) {
            if (q < MN_NUM_ACTIONS) {
                const size_t at = (size_t)i * MN_NUM_ACTIONS + q;
                if (R.scores) R.scores[at] = ok ? score : __builtin_nan("");
                if (R.steps) R.steps[at] = ok ? n : 0;
                if (R.infos) R.infos[at] = (uint8_t)(ok ? info : flag);
            }
            if (q == 0) {
                if (R.actions) R.actions[i] = ok ? action : -1;
                if (R.flags) R.flags[i] = (uint8_t)flag;
            }
        }
    }
}

struct MnpTrace {
    float *obs;        // [T][n][26]
    float *reward;     // [T][n]
    uint8_t *done;     // [T][n]
    uint8_t *info;     // [T][n]
    int32_t *action;   // [T][n]
};

__global__ __launch_bounds__(MN_WAVE, 1) void mn_rollout_pilot_kernel(MnArrays A, MnDev P, int n_steps, const double *__restrict__ T_dev,
                                                                      const int32_t *__restrict__ field_of, long long n_fields, int nx, int ny, int H,
                                                                      float *__restrict__ obs_io, MnpTrace T, double *__restrict__ traj_trace) {
    static_assert(MN_STEP_BLOCK == MN_WAVE, "one wavefront per workgroup: the step's work-list hand-off is a wavefront's");
    constexpr int L = MNP_ROW;
    using Lane = MnLane<double, true, L>;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = tid / L, q = tid % L;
    const size_t n = (size_t)A.n, nc = (size_t)nx * ny;
    if (tid < 2 * MN_QSHARDS) A.queue_count[tid * MN_QSTRIDE] = 0u;      // as every episode kernel: nothing is left for a later mn_reset_done
    const MnRing none = {};
    Lane ln;
    ln.load(A, e, q);
    const bool exists = ln.active;
    // the env's field: a bad index or a BAD_ENV field (T[0] is NaN) poisons the env at its first step
    const double *Tf = T_dev;
    bool field_ok = false;
    if (exists) {
        const long long f = field_of ? (long long)field_of[e] : (long long)e;
        field_ok = f >= 0 && f < n_fields;
        if (field_ok) { Tf = T_dev + (size_t)f * nc; const double t0 = Tf[0]; field_ok = t0 == t0; }
    }
    bool alive = exists;
    int last_info = 0;
    for (int t = 0; t < n_steps; ++t) {
        const MnqRobot r0 = {ln.x, ln.y, ln.theta, ln.speed, 0.0, 0.0};
        const bool poisoned = alive && !(field_ok && mnq_state_ok(r0));
        const bool stepping = alive && !poisoned;
        double score;
        int n_a, info_a;
        int action = mnp_row_act(A, P, stepping, q, stepping ? e : 0, Tf, nx, ny, H, r0, ln.ep_t, score, n_a, info_a);
        action = stepping ? action : 0;
        float *orow = obs_io + (size_t)(exists ? e : 0) * MN_OBS_DIM;
        float *trow = T.obs ? T.obs + ((size_t)t * n + (exists ? e : 0)) * MN_OBS_DIM : nullptr;
        // traj_trace [T][n][N][2] (mn_set_trajectory_trace): the step body records env e's N sub-step positions at [e][s] of this step's slice
        if (traj_trace) { A.traj = stepping ? traj_trace + (size_t)t * n * (size_t)P.N * 2 : nullptr; A.traj_n = P.N; }
        ln.active = stepping;      // every store of the step is behind `active`: a finished env's lanes only keep the wavefront whole
        const MnStepOut o = ln.template step<false>(A, P, action, orow, (A.obs64 && stepping) ? A.obs64 + (size_t)e * MN_OBS_DIM : nullptr, none, nullptr,
                                                    nullptr, trow);
        if (exists && q == 0) {
            const size_t k = (size_t)t * n + e;
            if (T.reward) T.reward[k] = stepping ? (float)o.reward : 0.f;
            if (T.done) T.done[k] = stepping ? (uint8_t)o.done : (uint8_t)1;
            if (T.info) T.info[k] = stepping ? (uint8_t)o.info : (uint8_t)(poisoned ? MN_QUERY_INFO_BAD_STATE : last_info);
            if (T.action) T.action[k] = stepping ? action : -1;
        }
        if (stepping && o.done) {      // terminal pose and counters of this env are final (its observation row is already in obs_io)
            ln.store(A);
            last_info = o.info;
            alive = false;
        }
        if (poisoned) { last_info = MN_QUERY_INFO_BAD_STATE; alive = false; }
        if (!__any(alive)) {      // the whole wave is done: fill the remaining trace entries and leave
            for (int t2 = t + 1; t2 < n_steps; ++t2)
                if (exists && q == 0) {
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
        ln.active = true;
        ln.store(A);
    }
}

}  // namespace

void mn_launch_pilot_act(const MnArrays &A, const MnDev &P, const int32_t *env_of, int env0, const double *state, const int32_t *ep_t, const double *T,
                         const int32_t *field_of, int64_t n_fields, int nx, int ny, int horizon, int64_t nq, int32_t *actions, double *scores,
                         int32_t *steps, uint8_t *infos, uint8_t *flags, hipStream_t s) {
    const MnpActArgs R = {env_of, env0, state, ep_t, T, field_of, (long long)n_fields, nx, ny, horizon, (long long)nq, actions, scores, steps, infos, flags};
    const int64_t rows = MNP_BLOCK / MNP_ROW, b = (nq + rows - 1) / rows;
    hipLaunchKernelGGL(mn_pilot_act_kernel, dim3((unsigned)(b < 65536 ? b : 65536)), dim3(MNP_BLOCK), 0, s, A, P, R);
}

void mn_launch_rollout_pilot(const MnArrays &A, const MnDev &P, int n_steps, const double *T, const int32_t *field_of, int64_t n_fields, int nx, int ny,
                             int horizon, float *obs_io, float *obs_trace, float *reward_trace, uint8_t *done_trace, uint8_t *info_trace,
                             int32_t *action_trace, double *traj_trace, hipStream_t s) {
    const MnpTrace Tr = {obs_trace, reward_trace, done_trace, info_trace, action_trace};
    hipLaunchKernelGGL(mn_rollout_pilot_kernel, dim3((unsigned)((size_t)A.npad * MNP_ROW / MN_WAVE)), dim3(MN_WAVE), 0, s, A, P, n_steps, T, field_of,
                       (long long)n_fields, nx, ny, horizon, obs_io, Tr, traj_trace);
}
