// mn_done_queue.h -- what a queue-driven reset wavefront needs around mn_reset_env (mn_reset_body.h): the handle's sharded done-queue as the wavefront
// reads it, and the decaying peak of the episode counts the host decides with.  Shared by mn_reset.hip and mn_prep_reset.hip.
#pragma once
#include "mn_internal.h"

// `seen` (may be NULL): {device word, host-mapped word}.  Every queue-driven reset launch updates a decaying peak of the number of episodes it starts,
// peak <- max(count, peak - peak / 8), in the device word and copies it to the host-mapped one, which the host reads WITHOUT synchronising: its estimate
// of how many episodes end per vector step (mn_reset_done_async decides with it where the next reset runs).  Launches of one handle are sequential.
struct MnSeen { uint32_t *peak_dev; uint32_t *peak_host; };
__device__ __forceinline__ void mn_note_count(const MnSeen seen, uint32_t count) {
    if (seen.peak_dev && blockIdx.x == 0 && threadIdx.x == 0) {
        uint32_t p = *seen.peak_dev;
        p -= p >> 3;
        p = p > count ? p : count;
        *seen.peak_dev = p;
        __hip_atomic_store(seen.peak_host, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// The handle's done-queue of one step as a reset wavefront reads it (mn_internal.h: MN_QSHARDS lists, each with its own counter).  open(): lane s < 32 reads
// shard s's count, `incl` = inclusive prefix sum over the shards (kept in one register), returns the total.  at(qi): the qi-th finished env overall.
struct MnDoneQueue {
    uint32_t incl;
    __device__ __forceinline__ uint32_t open(const uint32_t *__restrict__ counts) {
        const int lane = threadIdx.x & (MN_WAVE - 1);
        uint32_t v = lane < MN_QSHARDS ? counts[lane * MN_QSTRIDE] : 0u;
#pragma unroll
        for (int off = 1; off < MN_QSHARDS; off <<= 1) {
            const uint32_t t = __shfl_up(v, off);
            if (lane >= off) v += t;
        }
        incl = v;
        return (uint32_t)__builtin_amdgcn_readlane((int)v, MN_QSHARDS - 1);
    }
    __device__ __forceinline__ int at(const int32_t *__restrict__ lists, int qcap, uint32_t qi) const {
        const int lane = threadIdx.x & (MN_WAVE - 1);
        const int sh = __popcll(__ballot(lane < MN_QSHARDS && incl <= qi));      // shards that end at or before entry qi
        const uint32_t before = sh ? (uint32_t)__builtin_amdgcn_readlane((int)incl, __builtin_amdgcn_readfirstlane(sh - 1)) : 0u;
        return lists[(size_t)sh * qcap + (qi - before)];
    }
};
