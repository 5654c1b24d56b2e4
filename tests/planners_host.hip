// planners_host.hip -- the device functions of csrc/mn_planners.h on the CPU: a stand-alone program for tests/test_planner_branches_cpu.py
// (hipcc --cuda-host-only -O2 -ffp-contract=off; the functions are __host__ __device__, so this is the arithmetic the kernels run, compiled for
// the host).  No GPU call is made.
//
//   planners_host IN OUT
// IN:  int32 n_rows, n_tables; double tables[n_tables][2][3] (a, w); float obs[n_rows][26].
// OUT: int8 act[n_tables][2][n_rows]: mn_policy_act of every (table, kind, row); kind 0 = MN_POLICY_APF, 1 = MN_POLICY_BA.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mn_planners.h"

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[2];
    if (fread(head, sizeof(head), 1, f) != 1) { fprintf(stderr, "short header\n"); return 2; }
    const int n = head[0], nt = head[1];
    if (n < 1 || nt < 1 || n > (1 << 24) || nt > 1024) { fprintf(stderr, "bad counts\n"); return 2; }
    std::vector<double> tables((size_t)nt * 6);
    std::vector<float> obs((size_t)n * MN_OBS_DIM);
    if (fread(tables.data(), sizeof(double), tables.size(), f) != tables.size() || fread(obs.data(), sizeof(float), obs.size(), f) != obs.size()) {
        fprintf(stderr, "short file\n"); return 2;
    }
    fclose(f);
    std::vector<int8_t> act((size_t)nt * 2 * n);
    const int kinds[2] = {MN_POLICY_APF, MN_POLICY_BA};
    for (int t = 0; t < nt; ++t) {
        MnPlanTabs T;
        for (int k = 0; k < 3; ++k) { T.a[k] = tables[(size_t)t * 6 + k]; T.w[k] = tables[(size_t)t * 6 + 3 + k]; }
        for (int kind = 0; kind < 2; ++kind)
            for (int i = 0; i < n; ++i)
                act[((size_t)t * 2 + kind) * n + i] = (int8_t)mn_policy_act(kinds[kind], &obs[(size_t)i * MN_OBS_DIM], T);
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (fwrite(act.data(), 1, act.size(), f) != act.size()) { fprintf(stderr, "short write\n"); return 2; }
    fclose(f);
    return 0;
}
