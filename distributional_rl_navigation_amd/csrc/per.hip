// per.hip -- proportional prioritized replay next to the device replay ring (gfx950): the priority store's append, the exact stratified sampler and the
// priority update.  The rule, operation by operation: include/marinenav_hip.h, "Prioritized replay"; its numpy / Python-int twin: tests/per_twin.py.
//
// A row's priority is an integer mass (uint32, MASS_ONE = 1 << 16 per unit); blocks of 1 024 consecutive rows carry a uint64 sum.  Integer sums are exact
// and independent of the order in which atomics land, so the sampler's answer is a function of the masses alone and a host twin can restate it bit for bit.
// Three small launches per gradient step (sample, the weighted step's forward / backward in iqn_train.hip, update) and one per ring write (append).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "marinenav_hip.h"
#include "mn_train_shared.h"

namespace {

constexpr int BLK = MN_PER_BLOCK;             // rows per block sum
constexpr int MAX_BLOCKS = MN_PER_MAX_CAPACITY / BLK;      // 1 024: one block sum per thread of the sampler's workgroup
constexpr int SAMPLE_THREADS = 1024;
constexpr int N_WAVES = SAMPLE_THREADS / 64;
constexpr int PER_LANE = BLK / 64;            // a block's rows per lane of the wavefront that walks it
constexpr int NQ = 8;                         // taus per sample in training
constexpr uint64_t PER_KEY = 0x8CB92BA72F3D8DD7ull;       // the key of the stratum words, apart from the taus' (0xD1B5...) and the permutation's (0xA24B...)

typedef unsigned long long ull;

// iqn_train.hip's `sample_tau`: the gradient step's tau number e under the call's base
__device__ __forceinline__ float sample_tau(uint64_t base, int e) {
    const uint64_t x = mix64(base ^ (0xD1B54A32D192ED03ull * (uint64_t)(e + 1)));
    return (float)(x >> 40) * (1.0f / 16777216.0f);
}

// inclusive prefix sum over the 64 lanes of a wavefront
__device__ __forceinline__ uint64_t wave_scan(uint64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = (uint64_t)__shfl_up((ull)v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// rows [ptr, ptr + n) mod cap get mass *mmax; a wavefront whose rows share a block sends ONE atomic with the sum of its differences (the usual case: 64
// consecutive rows), otherwise one per row.  Differences are taken modulo 2^64: a block sum never leaves [0, 2^41).
__global__ __launch_bounds__(256) void per_append_kernel(uint32_t *__restrict__ mass, ull *__restrict__ bsum, const uint32_t *__restrict__ mmax, int64_t ptr,
                                                         int64_t n, int64_t cap) {
    const uint32_t m = *mmax;
    const int lane = threadIdx.x & 63;
    for (int64_t i0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) - lane; i0 < n; i0 += (int64_t)gridDim.x * blockDim.x) {      // (uniform per wavefront)
        const int64_t i = i0 + lane;
        const bool on = i < n;
        int64_t slot = ptr + (on ? i : 0);
        slot = slot >= cap ? slot - cap : slot;
        uint64_t diff = 0;
        if (on) {
            diff = (uint64_t)m - (uint64_t)mass[slot];
            mass[slot] = m;
        }
        const int64_t b = slot / BLK, b_first = __shfl(b, 0, 64);
        if (__all(!on || b == b_first)) {      // (lane 0 is always on)
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) diff += (uint64_t)__shfl_down((ull)diff, d, 64);
            if (lane == 0 && diff) atomicAdd(bsum + b_first, (ull)diff);
        } else if (on && diff) {
            atomicAdd(bsum + b, (ull)diff);
        }
    }
}

// The sampler: ONE workgroup of 16 wavefronts.  Exclusive scan of the block sums in LDS (8 KB), then one wavefront per slot: its stratum's target, the block by
// binary search in LDS, the row inside the block's 1 024 masses: every lane sums 16 consecutive rows, one wave prefix scan over the 64 sums names the lane,
// and that lane walks its 16 -- one wave scan per slot, not one per 64 rows: a slot is a chain of dependent steps, and wave scans are the longest of them.
__global__ __launch_bounds__(SAMPLE_THREADS) void per_sample_kernel(const uint32_t *__restrict__ mass, const ull *__restrict__ bsum, int64_t size, int64_t cap,
                                                                    int n_blocks, int batch, float beta, uint64_t *__restrict__ state,
                                                                    int64_t *__restrict__ idx_out, float *__restrict__ w_out, float *__restrict__ taus_out) {
    __shared__ uint64_t s_ex[MAX_BLOCKS];      // exclusive prefix of the block sums
    __shared__ uint64_t s_wave[N_WAVES];
    __shared__ float s_w[MN_PER_MAX_BATCH];
    __shared__ float s_wmax[N_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t ctr = state[1], base = sample_base(state);
    // ---- exclusive scan of the <= 1 024 block sums
    const uint64_t own = tid < n_blocks ? (uint64_t)bsum[tid] : 0;
    const uint64_t inc = wave_scan(own, lane);
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();      // (also: every thread has read the generator state)
    uint64_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < N_WAVES; ++w) {
        const uint64_t t = s_wave[w];
        if (w < wave) before += t;
        total += t;
    }
    s_ex[tid] = before + inc - own;
    __syncthreads();
    if (tid == 0) state[1] = ctr + 1;
    for (int e = tid; e < 2 * batch * NQ; e += SAMPLE_THREADS) taus_out[e] = sample_tau(base, e);      // the step's taus: mn_iqn_sample's
    // ---- the slots
    const uint64_t q = total / (uint64_t)batch;
    const float f_size = (float)size, f_total = (float)total;
    for (int k = wave; k < batch; k += N_WAVES) {
        const uint64_t u24 = mix64(base ^ (PER_KEY * (uint64_t)(k + 1))) >> 40;
        const uint64_t target = (uint64_t)k * q + __umul64hi(u24 << 40, q);
        // the last block whose exclusive prefix is <= target: its inclusive prefix exceeds target, no earlier block's does (empty blocks tie and lose)
        int lo = 0, hi = n_blocks - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_ex[mid] <= target) lo = mid; else hi = mid - 1;
        }
        const int64_t row0 = (int64_t)lo * BLK;
        const uint64_t rem = target - s_ex[lo];
        // lane l takes rows row0 + 16 l .. + 15 (four 16-byte loads, element by element only where the ring ends inside them)
        uint32_t mv[PER_LANE];
#pragma unroll
        for (int c4 = 0; c4 < PER_LANE; c4 += 4) {
            const int64_t r = row0 + lane * PER_LANE + c4;
            if (r + 4 <= cap) {
                const uint4 v = *reinterpret_cast<const uint4 *>(mass + r);
                mv[c4] = v.x; mv[c4 + 1] = v.y; mv[c4 + 2] = v.z; mv[c4 + 3] = v.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) mv[c4 + c] = r + c < cap ? mass[r + c] : 0u;
            }
        }
        uint64_t own_sum = 0;
#pragma unroll
        for (int c = 0; c < PER_LANE; ++c) own_sum += mv[c];
        const uint64_t upto = wave_scan(own_sum, lane);      // ONE wave prefix scan per slot, over the lanes' sums
        int64_t row = size - 1;      // (never kept while the block sums are the sums of the masses)
        uint32_t m_row = 1u;
        const ull hit = __ballot(upto > rem);
        if (hit) {      // uniform
            const int at = __ffsll(hit) - 1;      // the least lane whose inclusive prefix exceeds the remainder: the row is among its 16
            const uint64_t rem_l = rem - (upto - own_sum);      // (meaningful in lane `at`)
            uint64_t run = 0;
            int cc = -1;
            uint32_t mm = 0;
#pragma unroll
            for (int c = 0; c < PER_LANE; ++c) {
                run += mv[c];
                if (cc < 0 && run > rem_l) { cc = c; mm = mv[c]; }
            }
            row = row0 + at * PER_LANE + __shfl(cc, at, 64);
            m_row = (uint32_t)__shfl((int)mm, at, 64);
        }
        if (lane == 0) {
            idx_out[k] = row;
            s_w[k] = powf(f_size * (float)m_row / f_total, -beta);
        }
    }
    __syncthreads();
    // ---- importance weights over the batch's largest
    float wm = 0.f;
    for (int k = tid; k < batch; k += SAMPLE_THREADS) wm = fmaxf(wm, s_w[k]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) wm = fmaxf(wm, __shfl_xor(wm, d, 64));
    if (lane == 0) s_wmax[wave] = wm;
    __syncthreads();
    wm = s_wmax[0];
#pragma unroll
    for (int w = 1; w < N_WAVES; ++w) wm = fmaxf(wm, s_wmax[w]);
    for (int k = tid; k < batch; k += SAMPLE_THREADS) w_out[k] = s_w[k] / wm;
}

// The update: ONE workgroup, thread k = slot k.  A row named by several slots is written by the highest of them only, so every row has one writer and the block
// sums move by the difference to the mass that writer read.
__global__ __launch_bounds__(SAMPLE_THREADS) void per_update_kernel(uint32_t *__restrict__ mass, ull *__restrict__ bsum, uint32_t *__restrict__ mmax,
                                                                    const int64_t *__restrict__ idx, const float *__restrict__ absdelta, int batch, float alpha,
                                                                    float eps, int64_t cap) {
    __shared__ int s_idx[MN_PER_MAX_BATCH];
    const int k = threadIdx.x;
    int64_t row = -1;
    if (k < batch) {
        row = idx[k];
        if (row < 0 || row >= cap) row = -1;      // (a row outside the ring is dropped, never written)
        s_idx[k] = (int)row;
    }
    __syncthreads();
    if (row < 0) return;
    bool later = false;      // (no early exit: the reads of a thread are independent and go out together)
#pragma unroll 8
    for (int j = k + 1; j < batch; ++j) later |= s_idx[j] == (int)row;
    if (later) return;
    const float v = floorf(powf(absdelta[k] + eps, alpha) * 65536.0f + 0.5f);
    uint32_t m = 1u;
    if (v >= 2147483648.0f) m = 0x7fffffffu;
    else if (v >= 1.0f) m = (uint32_t)v;      // (NaN: 1)
    const uint32_t old = mass[row];
    mass[row] = m;
    const uint64_t diff = (uint64_t)m - (uint64_t)old;
    if (diff) atomicAdd(bsum + row / BLK, (ull)diff);
    atomicMax(mmax, m);
}

}  // namespace

extern "C" int mn_per_append(uint32_t *mass, uint64_t *block_sums, const uint32_t *mmax, int64_t ptr, int64_t n, int64_t capacity, void *stream) {
    if (!mass || !block_sums || !mmax) return MN_ERR_INVALID;
    if (capacity <= 0 || capacity > MN_PER_MAX_CAPACITY || ptr < 0 || ptr >= capacity || n <= 0 || n > capacity) return MN_ERR_INVALID;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(per_append_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mass, reinterpret_cast<ull *>(block_sums), mmax, ptr, n, capacity);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

extern "C" int mn_per_sample(const uint32_t *mass, const uint64_t *block_sums, int64_t size, int64_t capacity, int32_t batch, float beta,
                             uint64_t *rng_state_dev, int64_t *idx_out, float *weights_out, float *taus_out, void *stream) {
    if (!mass || !block_sums || !rng_state_dev || !idx_out || !weights_out || !taus_out) return MN_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(mass) & 15) return MN_ERR_INVALID;      // (the sampler reads masses 16 bytes at a time)
    if (capacity <= 0 || capacity > MN_PER_MAX_CAPACITY || batch <= 0 || batch > MN_PER_MAX_BATCH || size < batch || size > capacity) return MN_ERR_INVALID;
    if (!(beta >= 0.f)) return MN_ERR_INVALID;
    const int n_blocks = (int)((capacity + BLK - 1) / BLK);
    hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, mass, reinterpret_cast<const ull *>(block_sums), size, capacity,
                       n_blocks, batch, beta, rng_state_dev, idx_out, weights_out, taus_out);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

extern "C" int mn_per_update(uint32_t *mass, uint64_t *block_sums, uint32_t *mmax, const int64_t *idx_dev, const float *absdelta_dev, int32_t batch,
                             float alpha, float eps, int64_t capacity, void *stream) {
    if (!mass || !block_sums || !mmax || !idx_dev || !absdelta_dev) return MN_ERR_INVALID;
    if (capacity <= 0 || capacity > MN_PER_MAX_CAPACITY || batch <= 0 || batch > MN_PER_MAX_BATCH) return MN_ERR_INVALID;
    hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(SAMPLE_THREADS), 0, (hipStream_t)stream, mass, reinterpret_cast<ull *>(block_sums), mmax, idx_dev, absdelta_dev,
                       batch, alpha, eps, capacity);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}
