// render_host.hip -- the raster rules of csrc/mn_render_body.h on the CPU: a stand-alone program for tests/test_render_cpu.py and the reference of
// tests/test_render_gpu.py (hipcc --cuda-host-only -ffp-contract=off; the body is __host__ __device__, so this is the arithmetic the kernels run,
// compiled for the host).  No GPU call is made.
//
//   render_host IN OUT
// IN:  int32 n_images, width, height, n_prims, render, uint32 fill, int32 0, 0; double view[4]; mn_params (raw); mn_render_style (raw); n_images
//      records of int32 n_cores, n_obs (n_cores < 0: no such world); double cores[8][3] (x, y, +Gamma if clockwise else -Gamma), obstacles[10][3]
//      (x, y, r), start[2], goal[2]; n_prims records of mn_render_prim.
//      render != 0: the images are what mn_render_worlds gives; else every pixel starts as `fill`.  Then the primitives are drawn, in order.
// OUT: uint32 [n_images][height][width]; int64 the work items the primitives had (samples of segments, box pixels of discs and rings, over
//      all their images), int64 the largest number of items any one primitive had in one image.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "mn_render_body.h"

struct WorldRec {
    int32_t nc, no;
    double cores[MN_MAX_CORES][3], obst[MN_MAX_OBS][3], start[2], goal[2];
};
struct HostWorld {
    const double (*o)[3];
    void obstacle(int k, double &x, double &y, double &r) const { x = o[k][0]; y = o[k][1]; r = o[k][2]; }
};
struct HostPalette {
    const uint32_t *pal;
    uint32_t operator()(int level) const { return pal[level]; }
};
struct HostPut {
    uint32_t *image;
    int W, H;
    uint32_t word;
    void operator()(int c, int r) {
        if (c < 0 || c >= W || r < 0 || r >= H) { fprintf(stderr, "a primitive left the image: (%d, %d)\n", c, r); exit(3); }
        uint32_t &px = image[(size_t)r * W + c];
        if (word > px) px = word;
    }
};

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t head[8];
    double view[4];
    mn_params p;
    mn_render_style S;
    if (fread(head, sizeof(head), 1, f) != 1 || fread(view, sizeof(view), 1, f) != 1 || fread(&p, sizeof(p), 1, f) != 1 || fread(&S, sizeof(S), 1, f) != 1) {
        fprintf(stderr, "short header\n"); return 2;
    }
    const int n_images = head[0], W = head[1], H = head[2], n_prims = head[3], render = head[4];
    const uint32_t fill = (uint32_t)head[5];
    if (n_images < 1 || W < 1 || H < 1 || n_prims < 0 || (int64_t)n_images * W * H >= ((int64_t)1 << 31) || !(view[2] > view[0]) || !(view[3] > view[1]) ||
        S.n_levels < 1 || S.n_levels > MN_RENDER_MAX_LEVELS || S.lic_steps < 0 || S.lic_steps > MN_RENDER_MAX_LIC_STEPS || S.lic_floor < 0 ||
        S.lic_floor > 255 || !(S.v_max > 0.0)) {
        fprintf(stderr, "arguments mn_render_worlds would refuse\n"); return 2;
    }
    std::vector<WorldRec> worlds((size_t)n_images);
    std::vector<mn_render_prim> prims((size_t)n_prims);
    if (fread(worlds.data(), sizeof(WorldRec), worlds.size(), f) != worlds.size() ||
        (n_prims && fread(prims.data(), sizeof(mn_render_prim), prims.size(), f) != prims.size())) {
        fprintf(stderr, "short file\n"); return 2;
    }
    fclose(f);
    MnDev P;      // the fields the body reads, as mn_capi.hip's derive() forms them
    memset(&P, 0, sizeof(P));
    P.width = p.width; P.height = p.height; P.core_r = p.core_r; P.goal_dis = p.goal_dis;
    P.two_pi = 2 * M_PI;
    P.two_pi_r_r = 2 * M_PI * p.core_r * p.core_r;
    const MnrView V = mnr_view(view, W, H);
    std::vector<uint32_t> px((size_t)n_images * W * H, fill);
    if (render) {
        const HostPalette pal = {S.palette};
        for (int i = 0; i < n_images; ++i) {
            const WorldRec &r = worlds[i];
            uint32_t *img = &px[(size_t)i * W * H];
            if (r.nc < 0) { for (int k = 0; k < W * H; ++k) img[k] = S.outside & 0xffffffu; continue; }
            if (r.nc > MN_MAX_CORES || r.no < 0 || r.no > MN_MAX_OBS) { fprintf(stderr, "world %d: bad counts\n", i); return 2; }
            MnqCores C;
            C.nc = r.nc;
            for (int k = 0; k < MN_MAX_CORES; ++k) { C.cx[k] = r.cores[k][0]; C.cy[k] = r.cores[k][1]; C.cg[k] = r.cores[k][2]; }
            const HostWorld w = {r.obst};
            for (int row = 0; row < H; ++row)
                for (int c = 0; c < W; ++c)
                    img[(size_t)row * W + c] = mnr_world_pixel(C, w, r.no, r.start[0], r.start[1], r.goal[0], r.goal[1], P, V, S, pal, c, row);
        }
    }
    int64_t items = 0, most = 0;
    for (int k = 0; k < n_prims; ++k) {
        MnrPlan L;
        if (!mnr_plan(prims[k], V, n_images, L)) continue;
        if (L.per_image > most) most = L.per_image;
        for (int i = L.i0; i <= L.i1; ++i) {
            HostPut put = {&px[(size_t)i * W * H], W, H, L.word};
            for (long long j = 0; j < L.per_image; ++j) mnr_item(L, V, j, put);
            items += L.per_image;
        }
    }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 2; }
    const int64_t tail[2] = {items, most};
    if (fwrite(px.data(), 4, px.size(), f) != px.size() || fwrite(tail, sizeof(tail), 1, f) != 1) { fprintf(stderr, "short write\n"); return 2; }
    fclose(f);
    return 0;
}
