// mn_obs_noise_body.h -- the observation-noise rule of include/marinenav_hip.h ("Observation noise"), operation by operation.
// __host__ __device__: mn_obs_noise.hip (mn_obs_perturb), the episode kernels' NOISE instantiations and tests/obs_noise_host.hip (the CPU build the
// numpy twin tests/obs_noise_twin.py is held to, word for word) all compile THIS text.  Integers make every draw; float32 throughout, every product and
// sum rounded on its own: the pragma inside each function body holds whatever -ffp-contract the including file is built with, and ends with the body.
#pragma once
#include <stdint.h>

#include "marinenav_hip.h"

#ifndef MNN_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define MNN_HD __host__ __device__ __forceinline__
#else
#define MNN_HD inline
#endif
#endif

#define MN_OBS_NOISE_ROW_KEY 0xC2B2AE3D27D4EB4Full      // keys of this rule alone (apart from the taus', the permutation's, PER's and exploration's)
#define MN_OBS_NOISE_CHANNEL_KEY 0x165667B19E3779F9ull
#define MN_OBS_NOISE_CHANNELS 15                        // velocity x, y | goal x, y | eleven beams
#define MN_OBS_NOISE_Z_SCALE 0x1.bb67aep-16f            // float32(1 / sqrt((2^32 - 1) / 3)): the centred sum of four 16-bit words to unit variance

// The description as the kernels take it: the public one with the miss probability turned into the 24-bit threshold (mn_obs_noise_dev_of).
struct MnObsNoiseDev {
    uint64_t seed;
    float vel_sigma, goal_sigma, sonar_rel_sigma;
    uint32_t miss_thr;      // a beam with a return reports none iff its 24-bit miss word < miss_thr; 0 = never, 2^24 = always
};

// ... and as an episode kernel takes it: with the handle's first_env_index
struct MnObsNoiseArg {
    MnObsNoiseDev S;
    uint64_t env0;
};

MNN_HD uint64_t mn_obs_noise_mix64(uint64_t x) {      // splitmix64 finaliser: the library's mix64
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// key of one observation: (seed, global env index, episode_timesteps when the observation was made)
// (in two halves: an episode kernel forms an env's half once, in front of its step loop)
MNN_HD uint64_t mn_obs_noise_env_key(uint64_t seed, uint64_t env) { return mn_obs_noise_mix64(seed + 0x9E3779B97F4A7C15ull * (env + 1)); }
MNN_HD uint64_t mn_obs_noise_step_key(uint64_t env_key, uint64_t ep_t) { return mn_obs_noise_mix64(env_key ^ (MN_OBS_NOISE_ROW_KEY * (ep_t + 1))); }
MNN_HD uint64_t mn_obs_noise_row_key(uint64_t seed, uint64_t env, uint64_t ep_t) {
    return mn_obs_noise_step_key(mn_obs_noise_env_key(seed, env), ep_t);
}
// word `w` (0: the normal stand-in's, 1: the miss word's) of channel `c`
MNN_HD uint64_t mn_obs_noise_word(uint64_t row_key, int c, int w) {
    return mn_obs_noise_mix64(row_key ^ (MN_OBS_NOISE_CHANNEL_KEY * (uint64_t)(2 * c + w + 1)));
}
// standard-normal stand-in: the four 16-bit fields of a word summed (an integer in [0, 262 140]), centred (- 131 070: |.| < 2^18, exact in float32),
// times one float32 constant.  Support +-3.464.
MNN_HD float mn_obs_noise_z(uint64_t word) {
#pragma clang fp contract(off)
    const int32_t s = (int32_t)(word & 0xFFFFu) + (int32_t)((word >> 16) & 0xFFFFu) + (int32_t)((word >> 32) & 0xFFFFu) + (int32_t)(word >> 48);
    return (float)(s - 131070) * MN_OBS_NOISE_Z_SCALE;
}

// Channel c of one row: reads in[] and writes out[] at the channel's own one or two elements only (c < 4: element c; else elements 4 + 2 (c - 4) and
// the next), so out == in is allowed and channels may run on different lanes.  A channel whose parameter is zero copies the words.
MNN_HD void mn_obs_noise_channel(const float *in, float *out, int c, uint64_t row_key, const MnObsNoiseDev S) {
#pragma clang fp contract(off)
    const float vel_sigma = S.vel_sigma, goal_sigma = S.goal_sigma, sonar_rel_sigma = S.sonar_rel_sigma;
    const uint32_t miss_thr = S.miss_thr;
    if (c < 4) {
        const float sigma = c < 2 ? vel_sigma : goal_sigma;
        float v = in[c];
        if (sigma != 0.0f) {
            const float d = sigma * mn_obs_noise_z(mn_obs_noise_word(row_key, c, 0));
            v = v + d;
        }
        out[c] = v;
        return;
    }
    const int k = 4 + 2 * (c - 4);
    float x = in[k], y = in[k + 1];
    if (!(x == 0.0f && y == 0.0f)) {      // (0, 0) is "no reflection": left as it is, sign bits included
        if (miss_thr != 0u && (uint32_t)(mn_obs_noise_word(row_key, c, 1) >> 40) < miss_thr) {
            x = 0.0f;
            y = 0.0f;
        } else if (sonar_rel_sigma != 0.0f) {
            const float d = sonar_rel_sigma * mn_obs_noise_z(mn_obs_noise_word(row_key, c, 0));
            const float f = 1.0f + d;
            x = x * f;
            y = y * f;
        }
    }
    out[k] = x;
    out[k + 1] = y;
}

// Host side: the public description validated and turned into the kernels' form.  NULL = valid, else the name of the offending parameter.
static inline const char *mn_obs_noise_dev_of(const mn_obs_noise &s, MnObsNoiseDev *out) {
    const float sig[3] = {s.vel_sigma, s.goal_sigma, s.sonar_rel_sigma};
    const char *names[3] = {"vel_sigma", "goal_sigma", "sonar_rel_sigma"};
    for (int i = 0; i < 3; ++i)
        if (!(sig[i] >= 0.0f) || __builtin_isinf(sig[i])) return names[i];      // negative, NaN or infinite
    if (!(s.sonar_miss_p >= 0.0f && s.sonar_miss_p <= 1.0f)) return "sonar_miss_p";
    out->seed = s.seed;
    out->vel_sigma = s.vel_sigma; out->goal_sigma = s.goal_sigma; out->sonar_rel_sigma = s.sonar_rel_sigma;
    out->miss_thr = (uint32_t)((double)s.sonar_miss_p * 16777216.0);      // exact product, truncated: p = 1 -> 2^24, every word is below it
    return nullptr;
}
static inline bool mn_obs_noise_is_off(const MnObsNoiseDev &d) {
    return d.vel_sigma == 0.0f && d.goal_sigma == 0.0f && d.sonar_rel_sigma == 0.0f && d.miss_thr == 0u;
}
