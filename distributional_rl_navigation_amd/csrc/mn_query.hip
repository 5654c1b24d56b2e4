// mn_query.hip -- mn_query_velocity / mn_query_observation (gfx950): the current field and the observation at poses the caller
// names, in worlds the handle holds, without stepping anything (arithmetic: mn_query_body.h).
//
// Mapping: one lane per query, 256-lane workgroups, a grid-stride loop over the queries (Q = 1 and Q = 2^22 take the same code).
// A query is independent of every other one, so there is nothing to share between lanes: no LDS, no cross-lane traffic.
//   * UNIFORM (env_of_query == NULL: every query asks the same world -- a flow-field grid, a policy map): the world's index is a
//     kernel argument, so the address of a table row is the same in all 64 lanes.  The cores are read once per wavefront in front
//     of the loop (scalar loads: the world lives in scalar registers, not in 64 copies); the first pass over the obstacles walks
//     k = 0 .. n_obs - 1 in step, one address per wavefront again; the reads inside a beam's scan (obstacle k of THIS lane's
//     reach list) are vector loads whose lanes fall on the same ten rows -- a broadcast out of one or two cache lines.
//   * per-query worlds: lane q reads rows [k][env] of the SoA tables for its own env (a gather; adjacent queries of adjacent
//     envs coalesce).  An index outside [0, n) reads nothing: NaN outputs, flag MN_QUERY_FLAG_BAD_ENV.
// The kernels only READ the handle's arrays; their stores go to the caller's output buffers alone.
#include "mn_query_body.h"

#define MNQ_BLOCK 256
#define MNQ_MAX_BLOCKS 2048      // 8 workgroups per CU of a 256-CU device; more queries than that: the stride loop

__device__ __forceinline__ void mnq_load_cores(const MnArrays &A, int e, MnqCores &W) {
    const int np = A.npad;
    W.nc = A.counts[e] & 0xff;
#pragma unroll
    for (int k = 0; k < MN_MAX_CORES; ++k) {
        W.cx[k] = A.cx[(size_t)k * np + e]; W.cy[k] = A.cy[(size_t)k * np + e]; W.cg[k] = A.cg[(size_t)k * np + e];
    }
}

// obstacle k of env e, straight from the master tables ([k][npad]); k < MN_MAX_OBS and e < n are the caller's
struct MnqObstacles {
    const double *__restrict__ ox, *__restrict__ oy, *__restrict__ orad;
    int np, e;
    __device__ __forceinline__ void obstacle(int k, double &x, double &y, double &r) const {
        const size_t at = (size_t)k * np + e;
        x = ox[at]; y = oy[at]; r = orad[at];
    }
};

template <bool UNIFORM>
__global__ __launch_bounds__(MNQ_BLOCK) void mn_query_velocity_kernel(const MnArrays A, const MnDev P, const int32_t *__restrict__ env_of, int env0,
                                                                      const double *__restrict__ xy, long long nq, double *__restrict__ v) {
    MnqCores W;
    if (UNIFORM) mnq_load_cores(A, env0, W);
    const long long stride = (long long)gridDim.x * MNQ_BLOCK;
    for (long long q = (long long)blockIdx.x * MNQ_BLOCK + threadIdx.x; q < nq; q += stride) {
        bool ok = true;
        if (!UNIFORM) {
            const int e = env_of[q];
            ok = e >= 0 && e < A.n;
            if (ok) mnq_load_cores(A, e, W);
        }
        const double x = xy[2 * q], y = xy[2 * q + 1];
        double vx = __builtin_nan(""), vy = __builtin_nan("");
        if (ok) mnq_velocity(W, P, x, y, vx, vy);
        v[2 * q] = vx; v[2 * q + 1] = vy;
    }
}

// one observation row leaving as it is produced: float32 pairs and / or float64 values
struct MnqRowOut {
    float *o32;
    double *o64;
    __device__ __forceinline__ void pair(int at, double a, double b) {
        if (o32) *reinterpret_cast<float2 *>(o32 + at) = make_float2((float)a, (float)b);
        if (o64) { o64[at] = a; o64[at + 1] = b; }
    }
    __device__ __forceinline__ void head(double o0, double o1, double o2, double o3) { pair(0, o0, o1); pair(2, o2, o3); }
    __device__ __forceinline__ void beam(int i, double bx, double by) { pair(4 + 2 * i, bx, by); }
};

template <bool UNIFORM, bool FROM_CURRENT>
__global__ __launch_bounds__(MNQ_BLOCK) void mn_query_observation_kernel(const MnArrays A, const MnDev P, const int32_t *__restrict__ env_of, int env0,
                                                                         const double *__restrict__ state, long long nq, float *__restrict__ obs,
                                                                         double *__restrict__ obs64, uint8_t *__restrict__ flags) {
    MnqCores W;
    if (UNIFORM && FROM_CURRENT) mnq_load_cores(A, env0, W);
    const long long stride = (long long)gridDim.x * MNQ_BLOCK;
    for (long long q = (long long)blockIdx.x * MNQ_BLOCK + threadIdx.x; q < nq; q += stride) {
        const int e = UNIFORM ? env0 : env_of[q];
        MnqRowOut out;
        out.o32 = obs ? obs + q * MN_OBS_DIM : nullptr;
        out.o64 = obs64 ? obs64 + q * MN_OBS_DIM : nullptr;
        if (!UNIFORM && (e < 0 || e >= A.n)) {
            const double nan = __builtin_nan("");
            for (int i = 0; i < MN_OBS_DIM; i += 2) out.pair(i, nan, nan);
            if (flags) flags[q] = MN_QUERY_FLAG_BAD_ENV;
            continue;
        }
        const double *st = state + q * 6;
        const double x = st[0], y = st[1], theta = st[2], speed = st[3];
        double velx, vely;
        if (FROM_CURRENT) {      // Robot.reset_state (robot.py:79-87)
            if (!UNIFORM) mnq_load_cores(A, e, W);
            double cvx, cvy;
            mnq_velocity(W, P, x, y, cvx, cvy);
            velx = speed * cos(theta) + cvx;
            vely = speed * sin(theta) + cvy;
        } else {
            velx = st[4]; vely = st[5];
        }
        const MnqObstacles obst = {A.ox, A.oy, A.orad, A.npad, e};
        const unsigned f = mnq_observe(obst, (A.counts[e] >> 8) & 0xff, A.goal_x[e], A.goal_y[e], P, x, y, theta, velx, vely, out);
        if (flags) flags[q] = (uint8_t)f;
    }
}

static int mnq_blocks(int64_t nq) {
    const int64_t b = (nq + MNQ_BLOCK - 1) / MNQ_BLOCK;
    return (int)(b < MNQ_MAX_BLOCKS ? b : MNQ_MAX_BLOCKS);
}

void mn_launch_query_velocity(const MnArrays &A, const MnDev &P, const int32_t *env_of, int env0, const double *xy, int64_t nq, double *v, hipStream_t s) {
    const dim3 grid(mnq_blocks(nq)), block(MNQ_BLOCK);
    if (env_of) hipLaunchKernelGGL(mn_query_velocity_kernel<false>, grid, block, 0, s, A, P, env_of, env0, xy, (long long)nq, v);
    else hipLaunchKernelGGL(mn_query_velocity_kernel<true>, grid, block, 0, s, A, P, env_of, env0, xy, (long long)nq, v);
}

void mn_launch_query_observation(const MnArrays &A, const MnDev &P, const int32_t *env_of, int env0, const double *state, int from_current, int64_t nq,
                                 float *obs, double *obs64, uint8_t *flags, hipStream_t s) {
    const dim3 grid(mnq_blocks(nq)), block(MNQ_BLOCK);
#define MNQ_LAUNCH(U, F) hipLaunchKernelGGL((mn_query_observation_kernel<U, F>), grid, block, 0, s, A, P, env_of, env0, state, (long long)nq, obs, obs64, flags)
    if (env_of) { if (from_current) MNQ_LAUNCH(false, true); else MNQ_LAUNCH(false, false); }
    else { if (from_current) MNQ_LAUNCH(true, true); else MNQ_LAUNCH(true, false); }
#undef MNQ_LAUNCH
}
