// mn_state.hip -- snapshot and restore of an env handle in one launch (mn_state_save / mn_state_load; blob layout in mn_internal.h).
// A copy, with one exception: the done-queue's lists are saved in a canonical order (see below).  No floating-point arithmetic, no LDS, no atomics.  The
// MT19937 rows are 2.5 KB per env and dominate; they are contiguous over the n real envs in the handle and in the blob, so they move as one run of 128-bit
// vectors, consecutive lanes on consecutive vectors.  Everything else is struct-of-arrays with the env index fastest: one thread per env, every access
// coalesced across the wave.
#include "mn_internal.h"

#define ST_THREADS 256
#define ST_MAX_BLOCKS 2048      // 8 workgroups of 256 on each of 256 CUs; the loops stride over the grid

template <bool SAVE, typename T>
__device__ __forceinline__ void mv(T *in_handle, T *in_blob) {
    if (SAVE) *in_blob = *in_handle; else *in_handle = *in_blob;
}

template <bool SAVE>
__global__ __launch_bounds__(ST_THREADS) void mn_state_kernel(const MnArrays A, const MnStateHeader hdr, unsigned char *blob, uint32_t *peak_dev, uint32_t *seen_dev,
                                                              uint32_t *ready) {
    const int64_t T = (int64_t)gridDim.x * ST_THREADS, g = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    const int64_t n = A.n, npad = A.npad;

    // the header: the host's words as they came with the launch, the two peak words as the device has them now, zeros up to MN_STATE_HEADER_BYTES
    if (SAVE) {
        if (g == 0) {
            MnStateHeader *bh = (MnStateHeader *)blob;
            *bh = hdr;
            if (hdr.has_peak) { bh->peak = *peak_dev; bh->seen = *seen_dev; }
        }
        uint32_t *tail = (uint32_t *)(blob + sizeof(MnStateHeader));
        for (int64_t i = g; i < (int64_t)((MN_STATE_HEADER_BYTES - sizeof(MnStateHeader)) / 4); i += T) tail[i] = 0u;
    } else {
        if (g == 0 && peak_dev) *peak_dev = hdr.peak;
        if (ready) for (int64_t i = g; i < npad; i += T) ready[i] = 0u;
    }

    // MT rows: n * 156 vectors of 128 bits
    unsigned char *p = blob + MN_STATE_HEADER_BYTES;
    {
        uint4 *bm = (uint4 *)p, *hm = (uint4 *)A.mt;
        const int64_t nv = n * (MN_STATE_MT_WORDS / 4);
        for (int64_t i = g; i < nv; i += T) mv<SAVE>(hm + i, bm + i);
        p += nv * 16;
    }
    // done-queue: both counter halves, then the shard lists
    {
        uint32_t *bq = (uint32_t *)p;
        for (int64_t i = g; i < 2 * MN_QWORDS; i += T) mv<SAVE>(A.queue_count + i, bq + i);
        p += 2 * MN_QWORDS * 4;
        int32_t *bl = (int32_t *)p;
        const int64_t nl = (int64_t)MN_QSHARDS * A.qcap;
        if (SAVE) {
            // Canonical lists.  The step kernel's waves append to a shard in whatever order they reach its counter, and what lies behind the count is left
            // over from earlier steps: neither is state (every listed env resets from its own stream), but both would make the blob's bytes depend on
            // wave timing.  So the blob gets, per shard, the live entries -- [0, count) of the half the last step filled -- in ascending order (rank by
            // comparison; ties, which a step never produces, by position) and zeros behind them.
            const uint32_t *cnt = A.queue_count + (int64_t)hdr.last_parity * MN_QWORDS;
            const int64_t qcap = A.qcap;
            for (int64_t i = g; i < nl; i += T) {
                const int64_t sh = i / qcap, k = i - sh * qcap;
                const uint32_t c0 = cnt[sh * MN_QSTRIDE];
                const int64_t c = c0 < (uint32_t)qcap ? (int64_t)c0 : qcap;
                if (k < c) {
                    const int32_t *row = A.queue + sh * qcap;
                    const int32_t v = row[k];
                    int64_t rank = 0;
                    for (int64_t j = 0; j < c; ++j) {
                        const int32_t w = row[j];
                        rank += (w < v || (w == v && j < k)) ? 1 : 0;
                    }
                    bl[sh * qcap + rank] = v;
                } else {
                    bl[i] = 0;
                }
            }
        } else {
            for (int64_t i = g; i < nl; i += T) A.queue[i] = bl[i];
        }
        p += nl * 4;
    }
    // per-env rows
    double *bd = (double *)p;
    int32_t *bi = (int32_t *)(p + (int64_t)MN_STATE_F64_ROWS * n * 8);
    for (int64_t e = g; e < n; e += T) {
        int r = 0;
#define ROW64(f) mv<SAVE>(A.f + e, bd + (int64_t)(r++) * n + e);
        ROW64(x) ROW64(y) ROW64(theta) ROW64(speed) ROW64(vx) ROW64(vy)
        ROW64(start_x) ROW64(start_y) ROW64(goal_x) ROW64(goal_y) ROW64(init_theta) ROW64(init_speed)
#undef ROW64
#define TAB64(f, K) _Pragma("unroll") for (int k = 0; k < K; ++k) mv<SAVE>(A.f + k * npad + e, bd + (int64_t)(r++) * n + e);
        TAB64(cx, MN_MAX_CORES) TAB64(cy, MN_MAX_CORES) TAB64(cg, MN_MAX_CORES)
        TAB64(ox, MN_MAX_OBS) TAB64(oy, MN_MAX_OBS) TAB64(orad, MN_MAX_OBS)
#undef TAB64
        mv<SAVE>(A.tot_t + e, (int64_t *)bd + (int64_t)(r++) * n + e);
        int q = 0;
        mv<SAVE>(A.ep_t + e, bi + (int64_t)(q++) * n + e);
        mv<SAVE>(A.counts + e, bi + (int64_t)(q++) * n + e);
        mv<SAVE>(A.mt_pos + e, bi + (int64_t)(q++) * n + e);
#define TAB32(f, K) _Pragma("unroll") for (int k = 0; k < K; ++k) mv<SAVE>((uint32_t *)A.f + k * npad + e, (uint32_t *)bi + (int64_t)(q++) * n + e);
        TAB32(qcx, MN_MAX_CORES) TAB32(qcy, MN_MAX_CORES) TAB32(qcg, MN_MAX_CORES)
        TAB32(qox, MN_MAX_OBS) TAB32(qoy, MN_MAX_OBS) TAB32(qor, MN_MAX_OBS)
#undef TAB32
    }
}

void mn_launch_state(bool save, const MnArrays &A, const MnStateHeader &hdr, void *blob, uint32_t *peak_dev, uint32_t *seen_dev, uint32_t *ready, hipStream_t s) {
    const int64_t work = (int64_t)A.n * (MN_STATE_MT_WORDS / 4);
    int64_t blocks = (work + ST_THREADS - 1) / ST_THREADS;
    if (blocks > ST_MAX_BLOCKS) blocks = ST_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    if (save) mn_state_kernel<true><<<dim3((unsigned)blocks), dim3(ST_THREADS), 0, s>>>(A, hdr, (unsigned char *)blob, peak_dev, seen_dev, ready);
    else mn_state_kernel<false><<<dim3((unsigned)blocks), dim3(ST_THREADS), 0, s>>>(A, hdr, (unsigned char *)blob, peak_dev, seen_dev, ready);
}
