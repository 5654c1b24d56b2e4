// mn_time_field.hip -- mn_time_field (gfx950): the least travel time to the goal from every cell of a grid over a world the handle holds, for a vehicle
// of constant speed carried by the current and kept out of the obstacles (rules and arithmetic: mn_time_field_body.h, include/marinenav_hip.h).
//
// Mapping: ONE workgroup per field, grid = number of fields; a field is a fixed point over its own cells only, so workgroups share nothing.  The
// workgroup has ceil(cells / 4) threads rounded up to whole wavefronts, at most 1 024 (4 cells per thread up to 4 096 cells, 16 at the 16 384-cell
// limit); thread t owns cells t, t + threads, t + 2 threads, ...: the lanes of a wavefront own consecutive cells of a row, so their 8-byte LDS reads of
// a neighbour (a constant offset away) fall on consecutive words -- 32 lanes x 8 B = the 64 banks once, no conflict -- and their global reads and
// stores are consecutive too.
//   LDS (dynamic): T [cells] f64, then the free flags [cells] u8 and two flag bytes per 64-cell chunk: 9 bytes per cell, 144.5 KB at the limit -- one
//     workgroup per CU there, 16 waves; a 32 x 32 field takes 9 KB and 256 threads, so eight of them share a CU.
//   workspace (global, the caller's, [fields][18][cells] f64): planes 0..15 the edge times of direction k, planes 16, 17 the cell currents.  The
//     edge times are computed ONCE: recomputing them per sweep would need the neighbours' currents in LDS (2 x 128 KB at the limit: no room) or 17
//     evaluations of the eight-core current per cell and sweep.  A sweep reads its 16 planes as consecutive 8-byte words, 2 MB per field at the limit.
// Phases: (a) current, free flag, source flag and T = 0 / +inf per owned cell; barrier.  (b) the 16 edge times of every owned cell, from the
// currents and flags of its neighbours.  (c) in-place PULL sweeps over the owned free cells -- only the owner writes a cell, every access to a field
// word is one aligned 8-byte LDS access (relaxed atomic load / store: a reader sees the old or the new word, both the time of a real path), a
// barrier with an OR of "some cell of mine fell" after each sweep; the loop ends at the first sweep without a change or at max_sweeps.  A wavefront
// skips a chunk of 64 cells none of whose neighbourhood fell in the sweep before (most sweeps move only a front).  (d, e) dir by
// one pass over the final field, T and dir stored.  Thread t reads in (c)-(e) only the edge times it wrote itself in (b), so no barrier separates
// (b) from (c).
// The kernel only READS the handle's arrays.
#include "mn_time_field_body.h"

#define MNTF_MAX_THREADS 1024
#define MNTF_PLANES (MNTF_DIRS + 2)

struct MntfObstacles {      // obstacle k of env e, straight from the master tables ([k][npad])
    const double *__restrict__ ox, *__restrict__ oy, *__restrict__ orad;
    int np, e;
    __device__ __forceinline__ void obstacle(int k, double &x, double &y, double &r) const {
        const size_t at = (size_t)k * np + e;
        x = ox[at]; y = oy[at]; r = orad[at];
    }
};

struct MntfGrid {
    double *T_;                  // LDS
    const unsigned char *fr;     // LDS
    const double *ws;            // this field's planes
    int nc;
    __device__ __forceinline__ bool free(int c) const { return fr[c] != 0; }
    __device__ __forceinline__ void current(int c, double &cx, double &cy) const { cx = ws[(size_t)MNTF_DIRS * nc + c]; cy = ws[(size_t)(MNTF_DIRS + 1) * nc + c]; }
    __device__ __forceinline__ double w(int k, int c) const { return ws[(size_t)k * nc + c]; }
    __device__ __forceinline__ double T(int c) const { return __hip_atomic_load(T_ + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ void setT(int c, double t) const { __hip_atomic_store(T_ + c, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

struct MntfPut {
    double *ws;
    int nc, c;
    __device__ __forceinline__ void operator()(int k, double w) { ws[(size_t)k * nc + c] = w; }
};

__global__ __launch_bounds__(MNTF_MAX_THREADS) void mn_time_field_kernel(const MnArrays A, const MnDev P, const int32_t *__restrict__ env_of, int env0,
                                                                         const double *__restrict__ goal_xy, int nx, int ny, double speed,
                                                                         double clearance, int max_sweeps, double *__restrict__ T_out,
                                                                         uint8_t *__restrict__ dir_out, int32_t *__restrict__ status,
                                                                         int32_t *__restrict__ sweeps_out, double *workspace) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int nc = nx * ny, f = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    double *To = T_out + (size_t)f * nc;
    uint8_t *Do = dir_out ? dir_out + (size_t)f * nc : nullptr;
    // which world, which goal: uniform over the workgroup, so the refusal below takes all of it
    const int e = env_of ? env_of[f] : env0;
    bool ok = e >= 0 && e < A.n;
    double gx = 0.0, gy = 0.0;
    if (ok) {
        gx = goal_xy ? goal_xy[2 * (size_t)f] : A.goal_x[e];
        gy = goal_xy ? goal_xy[2 * (size_t)f + 1] : A.goal_y[e];
        ok = (gx - gx == 0.0) && (gy - gy == 0.0);
    }
    if (!ok) {
        for (int c = tid; c < nc; c += nt) { To[c] = __builtin_nan(""); if (Do) Do[c] = MNTF_NO_DIR; }
        if (tid == 0) { status[f] = MN_TIME_FIELD_BAD_ENV; if (sweeps_out) sweeps_out[f] = 0; }
        return;
    }
    unsigned char *fr = reinterpret_cast<unsigned char *>(lds + nc);
    const int n_chunks = (nc + MN_WAVE - 1) / MN_WAVE;      // a chunk: the 64 consecutive cells one wavefront relaxes together
    unsigned char *fell_in = fr + (nc + 15) / 16 * 16;      // [2][n_chunks]: did a cell of the chunk fall in the last sweep of that parity
    double *ws = workspace + (size_t)f * MNTF_PLANES * nc;
    const MntfGrid g = {lds, fr, ws, nc};
    const double hx = P.width / (double)nx, hy = P.height / (double)ny;
    const double s = speed > 0.0 ? speed : P.max_speed;

    // (a)
    MnqCores W;
    {
        const int np = A.npad;
        W.nc = A.counts[e] & 0xff;
#pragma unroll
        for (int k = 0; k < MN_MAX_CORES; ++k) { W.cx[k] = A.cx[(size_t)k * np + e]; W.cy[k] = A.cy[(size_t)k * np + e]; W.cg[k] = A.cg[(size_t)k * np + e]; }
    }
    const MntfObstacles obst = {A.ox, A.oy, A.orad, A.npad, e};
    const int no = (A.counts[e] >> 8) & 0xff;
    int mine = 0;
    for (int c = tid; c < nc; c += nt) {
        const int j = c / nx, i = c - j * nx;
        double cx, cy;
        bool is_free, is_source;
        mntf_cell(W, obst, no, gx, gy, P, hx, hy, clearance, i, j, cx, cy, is_free, is_source);
        ws[(size_t)MNTF_DIRS * nc + c] = cx;
        ws[(size_t)(MNTF_DIRS + 1) * nc + c] = cy;
        fr[c] = is_free ? 1 : 0;
        lds[c] = is_source ? 0.0 : (double)INFINITY;
        mine |= is_source ? 1 : 0;
    }
    for (int ch = tid; ch < n_chunks; ch += nt) fell_in[ch] = 1;      // (in front of the first sweep everything is new)
    __threadfence_block();      // the currents go through global memory to the other threads of this workgroup
    const int has_source = __syncthreads_or(mine);

    // (b)
    for (int c = tid; c < nc; c += nt) {
        const int j = c / nx, i = c - j * nx;
        MntfPut put = {ws, nc, c};
        mntf_cell_edges(g, nx, ny, hx, hy, s, i, j, put);
    }

    // (c)  A wavefront relaxes a chunk only if a cell within two rows and two columns of it -- every neighbour of its cells lies there -- fell in the
    // sweep before: a cell whose neighbours have not fallen since it last looked still satisfies its equation.  The test is wave-uniform (the lanes
    // read the previous sweep's chunk flags, one vote), the flags of this sweep are written by the chunk's own wavefront, skipped chunks included.
    const int lane = tid & (MN_WAVE - 1), reach = 2 * nx + 2;
    int sweeps = 0, changed = has_source;
    while (changed && sweeps < max_sweeps) {
        const unsigned char *before = fell_in + (sweeps & 1) * n_chunks;
        unsigned char *now = fell_in + ((sweeps & 1) ^ 1) * n_chunks;
        int fell = 0;
        for (int base = tid - lane; base < nc; base += nt) {      // (base: the chunk's first cell, the same in all lanes)
            const int lo = base - reach, hi = base + MN_WAVE - 1 + reach;
            const int ch_lo = (lo < 0 ? 0 : lo) / MN_WAVE, ch_hi = (hi > nc - 1 ? nc - 1 : hi) / MN_WAVE;
            int near = 0;
            for (int ch = ch_lo + lane; ch <= ch_hi; ch += MN_WAVE) near |= before[ch];
            int mine_fell = 0;
            if (__any(near)) {
                const int c = base + lane;
                double t;
                if (c < nc && fr[c] && mntf_relax(g, nx, c, t)) { g.setT(c, t); mine_fell = 1; }
                mine_fell = __any(mine_fell);
            }
            if (lane == 0) now[base / MN_WAVE] = (unsigned char)mine_fell;
            fell |= mine_fell;
        }
        changed = __syncthreads_or(fell);
        ++sweeps;
    }

    // (d), (e)
    for (int c = tid; c < nc; c += nt) {
        To[c] = lds[c];
        if (Do) Do[c] = (uint8_t)mntf_dir(g, nx, c);
    }
    if (tid == 0) {
        status[f] = !has_source ? MN_TIME_FIELD_NO_SOURCE : (changed ? MN_TIME_FIELD_NOT_CONVERGED : MN_TIME_FIELD_OK);
        if (sweeps_out) sweeps_out[f] = sweeps;
    }
}

int64_t mn_time_field_planes_bytes(int nx, int ny, int64_t n_fields) { return n_fields * MNTF_PLANES * (int64_t)nx * ny * (int64_t)sizeof(double); }

int mn_launch_time_field(const MnArrays &A, const MnDev &P, const int32_t *env_of, int env0, const double *goal_xy, int64_t n_fields, int nx, int ny,
                         double speed, double clearance, int max_sweeps, double *T, uint8_t *dir, int32_t *status, int32_t *sweeps, void *workspace,
                         hipStream_t s) {
    const int nc = nx * ny;
    int threads = ((nc + 3) / 4 + MN_WAVE - 1) / MN_WAVE * MN_WAVE;
    threads = threads > MNTF_MAX_THREADS ? MNTF_MAX_THREADS : threads;
    const size_t lds_bytes = (size_t)nc * sizeof(double) + (size_t)(nc + 15) / 16 * 16 + 2 * (size_t)((nc + MN_WAVE - 1) / MN_WAVE);
    if (lds_bytes > 65536 && hipFuncSetAttribute(reinterpret_cast<const void *>(mn_time_field_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 MNTF_MAX_CELLS * 9 + 2 * MNTF_MAX_CELLS / MN_WAVE) != hipSuccess)      // (above 64 KB of dynamic LDS the runtime wants to be told)
        return MN_ERR_HIP;
    hipLaunchKernelGGL(mn_time_field_kernel, dim3((unsigned)n_fields), dim3(threads), lds_bytes, s, A, P, env_of, env0, goal_xy, nx, ny, speed, clearance,
                       max_sweeps, T, dir, status, sweeps, static_cast<double *>(workspace));
    return MN_OK;
}
