// time_field_host.hip -- the rules of csrc/mn_time_field_body.h on the CPU: a stand-alone program for tests/test_time_field_cpu.py and the reference of
// tests/test_time_field_gpu.py (hipcc --cuda-host-only -ffp-contract=off; the body is __host__ __device__, so this is the arithmetic the kernel runs,
// compiled for the host).  No GPU call is made.  The relaxation order is deliberately NOT the kernel's: plain row-major in-place sweeps over all
// cells, one after the other -- the field is a unique fixed point, so the order must not show.
//
//   time_field_host IN OUT
// IN:  int32 n_fields, nx, ny, max_sweeps; double speed, clearance; mn_params (raw); n_fields records of int32 n_cores, n_obs (n_cores < 0: no such
//      world); double cores[8][3] (x, y, +Gamma if clockwise else -Gamma), obstacles[10][3] (x, y, r), start[2] (unused), goal[2] (the goal of THIS
//      field: the world's own or the override; not finite: the field is refused like a bad world).
// OUT: double T [n_fields][ny][nx]; uint8 dir [n_fields][ny][nx]; int32 status [n_fields]; int32 sweeps [n_fields]; double current
//      [n_fields][ny][nx][2] (zeros for a refused field); double the seconds the solves took (wall clock, phases a-d of all fields).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "mn_time_field_body.h"

struct WorldRec {
    int32_t nc, no;
    double cores[MN_MAX_CORES][3], obst[MN_MAX_OBS][3], start[2], goal[2];
};
struct HostWorld {
    const double (*o)[3];
    void obstacle(int k, double &x, double &y, double &r) const { x = o[k][0]; y = o[k][1]; r = o[k][2]; }
};
struct HostGrid {
    const unsigned char *fr;
    const double *cur, *wk, *Tf;
    int nc;
    bool free(int c) const { return fr[c] != 0; }
    void current(int c, double &cx, double &cy) const { cx = cur[2 * c]; cy = cur[2 * c + 1]; }
    double w(int k, int c) const { return wk[(size_t)k * nc + c]; }
    double T(int c) const { return Tf[c]; }
};
struct HostPut {
    double *wk;
    int nc, c;
    void operator()(int k, double w) { wk[(size_t)k * nc + c] = w; }
};

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[4];
    double sc[2];
    mn_params p;
    if (fread(head, sizeof(head), 1, f) != 1 || fread(sc, sizeof(sc), 1, f) != 1 || fread(&p, sizeof(p), 1, f) != 1) { fprintf(stderr, "short header\n"); return 2; }
    const int n_fields = head[0], nx = head[1], ny = head[2], max_sweeps = head[3];
    const double speed = sc[0], clearance = sc[1];
    if (n_fields < 1 || nx < 1 || ny < 1 || (int64_t)nx * ny > MN_TIME_FIELD_MAX_CELLS || max_sweeps < 1 || !(clearance >= 0.0) || !(clearance - clearance == 0.0)) {
        fprintf(stderr, "arguments mn_time_field would refuse\n"); return 2;
    }
    std::vector<WorldRec> worlds((size_t)n_fields);
    if (fread(worlds.data(), sizeof(WorldRec), worlds.size(), f) != worlds.size()) { fprintf(stderr, "short file\n"); return 2; }
    fclose(f);
    MnDev P;      // the fields the body reads, as mn_capi.hip's derive() forms them
    memset(&P, 0, sizeof(P));
    P.width = p.width; P.height = p.height; P.core_r = p.core_r; P.goal_dis = p.goal_dis; P.robot_r = p.robot_r; P.max_speed = p.max_speed;
    P.two_pi = 2 * M_PI;
    P.two_pi_r_r = 2 * M_PI * p.core_r * p.core_r;
    const int nc = nx * ny;
    const double hx = P.width / (double)nx, hy = P.height / (double)ny;
    const double s = speed > 0.0 ? speed : P.max_speed;
    std::vector<double> T((size_t)n_fields * nc), cur((size_t)n_fields * nc * 2, 0.0), wk((size_t)MNTF_DIRS * nc);
    std::vector<uint8_t> dir((size_t)n_fields * nc), fr((size_t)nc);
    std::vector<int32_t> status((size_t)n_fields), sweeps((size_t)n_fields, 0);
    const auto t0 = std::chrono::steady_clock::now();
    for (int fi = 0; fi < n_fields; ++fi) {
        const WorldRec &r = worlds[fi];
        double *Tf = &T[(size_t)fi * nc], *cf = &cur[(size_t)fi * nc * 2];
        uint8_t *df = &dir[(size_t)fi * nc];
        const double gx = r.goal[0], gy = r.goal[1];
        if (r.nc < 0 || !(gx - gx == 0.0) || !(gy - gy == 0.0)) {
            for (int c = 0; c < nc; ++c) { Tf[c] = __builtin_nan(""); df[c] = MNTF_NO_DIR; }
            status[fi] = MN_TIME_FIELD_BAD_ENV;
            continue;
        }
        if (r.nc > MN_MAX_CORES || r.no < 0 || r.no > MN_MAX_OBS) { fprintf(stderr, "field %d: bad counts\n", fi); return 2; }
        MnqCores C;
        C.nc = r.nc;
        for (int k = 0; k < MN_MAX_CORES; ++k) { C.cx[k] = r.cores[k][0]; C.cy[k] = r.cores[k][1]; C.cg[k] = r.cores[k][2]; }
        const HostWorld w = {r.obst};
        bool has_source = false;
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                const int c = j * nx + i;
                bool is_free, is_source;
                mntf_cell(C, w, r.no, gx, gy, P, hx, hy, clearance, i, j, cf[2 * c], cf[2 * c + 1], is_free, is_source);
                fr[c] = is_free ? 1 : 0;
                Tf[c] = is_source ? 0.0 : (double)INFINITY;
                has_source = has_source || is_source;
            }
        const HostGrid g = {fr.data(), cf, wk.data(), Tf, nc};
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i) {
                HostPut put = {wk.data(), nc, j * nx + i};
                mntf_cell_edges(g, nx, ny, hx, hy, s, i, j, put);
            }
        bool changed = has_source;
        int n = 0;
        while (changed && n < max_sweeps) {
            changed = false;
            for (int c = 0; c < nc; ++c) {
                double t;
                if (fr[c] && mntf_relax(g, nx, c, t)) { Tf[c] = t; changed = true; }
            }
            ++n;
        }
        for (int c = 0; c < nc; ++c) df[c] = (uint8_t)mntf_dir(g, nx, c);
        status[fi] = !has_source ? MN_TIME_FIELD_NO_SOURCE : (changed ? MN_TIME_FIELD_NOT_CONVERGED : MN_TIME_FIELD_OK);
        sweeps[fi] = n;
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    if (fwrite(T.data(), 8, T.size(), f) != T.size() || fwrite(dir.data(), 1, dir.size(), f) != dir.size() ||
        fwrite(status.data(), 4, status.size(), f) != status.size() || fwrite(sweeps.data(), 4, sweeps.size(), f) != sweeps.size() ||
        fwrite(cur.data(), 8, cur.size(), f) != cur.size() || fwrite(&seconds, 8, 1, f) != 1) { fprintf(stderr, "short write\n"); return 2; }
    fclose(f);
    return 0;
}
