// obs_noise_host.hip -- the observation-noise rule (csrc/mn_obs_noise_body.h) on the CPU: a stand-alone program for tests/test_obs_noise_cpu.py
// (hipcc --cuda-host-only -ffp-contract=off; the body is __host__ __device__, so this is the arithmetic the kernels run, compiled for the host).
// No GPU call is made.
//
//   obs_noise_host IN OUT
// IN:  int64 n; mn_obs_noise (raw, 24 bytes); uint64 env[n]; int32 ep_t[n]; float rows[n][26].
// OUT: int32 status (0, or 1 + the index of the refused parameter: vel_sigma, goal_sigma, sonar_rel_sigma, sonar_miss_p), uint32 miss_thr; then, unless
//      refused, float rows[n][26] (the perceived rows); uint64 words[n][1 + 2 * 15] (row_key, then W(c, 0), W(c, 1) per channel); float z[n][15].
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mn_obs_noise_body.h"

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t n;
    mn_obs_noise spec;
    static_assert(sizeof(spec) == 24, "mn_obs_noise layout");
    if (fread(&n, 8, 1, f) != 1 || fread(&spec, sizeof(spec), 1, f) != 1 || n < 0 || n > (1 << 24)) { fprintf(stderr, "short header\n"); return 2; }
    std::vector<uint64_t> env((size_t)n);
    std::vector<int32_t> ep((size_t)n);
    std::vector<float> rows((size_t)n * MN_OBS_DIM), out((size_t)n * MN_OBS_DIM), z((size_t)n * MN_OBS_NOISE_CHANNELS);
    std::vector<uint64_t> words((size_t)n * (1 + 2 * MN_OBS_NOISE_CHANNELS));
    if (n && (fread(env.data(), 8, env.size(), f) != env.size() || fread(ep.data(), 4, ep.size(), f) != ep.size() ||
              fread(rows.data(), 4, rows.size(), f) != rows.size())) { fprintf(stderr, "short file\n"); return 2; }
    fclose(f);
    MnObsNoiseDev d = {};
    const char *bad = mn_obs_noise_dev_of(spec, &d);
    const char *names[4] = {"vel_sigma", "goal_sigma", "sonar_rel_sigma", "sonar_miss_p"};
    int32_t status = 0;
    for (int i = 0; bad && i < 4; ++i)
        if (!strcmp(bad, names[i])) status = 1 + i;
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    fwrite(&status, 4, 1, f);
    fwrite(&d.miss_thr, 4, 1, f);
    if (!status) {
        for (int64_t r = 0; r < n; ++r) {
            const uint64_t key = mn_obs_noise_row_key(d.seed, env[r], (uint64_t)(int64_t)ep[r]);
            uint64_t *w = &words[(size_t)r * (1 + 2 * MN_OBS_NOISE_CHANNELS)];
            w[0] = key;
            for (int c = 0; c < MN_OBS_NOISE_CHANNELS; ++c) {
                w[1 + 2 * c] = mn_obs_noise_word(key, c, 0);
                w[2 + 2 * c] = mn_obs_noise_word(key, c, 1);
                z[(size_t)r * MN_OBS_NOISE_CHANNELS + c] = mn_obs_noise_z(w[1 + 2 * c]);
                mn_obs_noise_channel(&rows[(size_t)r * MN_OBS_DIM], &out[(size_t)r * MN_OBS_DIM], c, key, d);
            }
        }
        if (n && (fwrite(out.data(), 4, out.size(), f) != out.size() || fwrite(words.data(), 8, words.size(), f) != words.size() ||
                  fwrite(z.data(), 4, z.size(), f) != z.size())) { fprintf(stderr, "short write\n"); return 2; }
    }
    fclose(f);
    return 0;
}
