// mn_train_shared.h -- device code shared by the two fused gradient steps (iqn_train.hip, dqn_train.hip): torch.optim.Adam's
// element update and the replay ring's batch draw.  Both steps must keep the arithmetic and the permutation of the other.
#pragma once

#include <stdint.h>

namespace {

// torch.optim.Adam's single-tensor update on one element: m.lerp_(g, 1 - b1); v.mul_(b2).addcmul_(g, g, value = 1 - b2); p.addcdiv_(m, sqrt(v) / bc2_sqrt + eps, value = -step_size)
__device__ __forceinline__ void adam_update(float g, float &m, float &v, float &p, float w1, float b2f, float w2, float step_size, float bc2_sqrt, float eps) {
    m = fmaf(g - m, w1, m);
    v = fmaf(w2, g * g, v * b2f);
    p = fmaf(-step_size, m / (sqrtf(v) / bc2_sqrt + eps), p);
}

// ---- the batch draw ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t x) {   // splitmix64 finaliser (Steele, Lea, Flood 2014)
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ uint32_t mix32(uint32_t x) {   // murmur3 finaliser
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    return x ^ (x >> 16);
}

// the key of the draw made at call counter `counter` of the generator seeded `seed`
__device__ __forceinline__ uint64_t sample_base_at(uint64_t seed, uint64_t counter) { return mix64(seed + 0x9E3779B97F4A7C15ull * (counter + 1)); }
__device__ __forceinline__ uint64_t sample_base(const uint64_t *__restrict__ state) { return sample_base_at(state[0], state[1]); }
// ReplayBuffer.sample (replay_buffer.py:42-47: random.sample(memory, k) = k DISTINCT uniform rows): slot k of the batch reads ring
// row perm(k), where perm is a pseudo-random permutation of [0, n) keyed by the step's `base` -- a 4-round balanced Feistel network
// on the smallest even-width power-of-two domain >= n (Luby-Rackoff: three rounds of a good round function already give a
// pseudo-random permutation), restricted to [0, n) by cycle walking (domain < 4 n: fewer than four evaluations expected).  The
// first `batch` images of a uniformly random permutation ARE a uniform sample without replacement; distinctness holds by
// construction, so a slot is O(1) and independent of the others -- every workgroup evaluates just its own two slots (round 2 ran
// a draw-and-redraw loop over the whole batch in every workgroup: 4-6 us of the kernel).
__device__ __forceinline__ uint32_t perm_row(uint64_t base, uint32_t n, uint32_t k) {
    const int bits = n > 1 ? 32 - __builtin_clz(n - 1) : 1;
    const int half = (bits + 1) >> 1;
    const uint32_t mask = (1u << half) - 1u;
    uint32_t rk[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) rk[r] = (uint32_t)(mix64(base + 0xA24BAED4963EE407ull * (uint64_t)(r + 1)) >> 32);
    uint32_t x = k;
    do {
        uint32_t L = x >> half, R = x & mask;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t t = L ^ (mix32(R + rk[r]) & mask);
            L = R;
            R = t;
        }
        x = (L << half) | R;
    } while (x >= n);
    return x;
}

}  // namespace
