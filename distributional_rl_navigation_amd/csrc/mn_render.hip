// mn_render.hip -- mn_render_worlds / mn_render_draw (gfx950): flow images of worlds the handle holds, and primitives drawn over images
// (rules: mn_render_body.h; stated in include/marinenav_hip.h).
//
// mn_render_worlds_kernel.  One 256-lane workgroup serves one image tile of 64 columns x 4 rows (lane = column, wavefront = row: a wavefront's
// stores are one 256-byte row segment), and takes its tiles from a stride loop over all tiles of all images, so the grid is bounded and one image and
// 4 000 images run the same code.  The tile, hence the image, hence the WORLD, is the same in all lanes of a workgroup: the world -- eight cores, ten
// obstacles, the counts, start and goal, 472 bytes -- is read from the handle's tables ONCE per (workgroup, image), one lane per word, into LDS, and
// every velocity evaluation and the obstacle pass (k in step) read it from there at wave-uniform addresses (a broadcast, no bank conflict).
// Everything else that is the same for the whole launch lives in LDS as well: the parameters, the view and the style with its palette (copied from
// the kernel argument block by the prologue, a word per lane), and the table pointers.  A per-lane level therefore indexes LDS, not a private array
// (which would be scratch), and the scalar file is left to the pixel loop's own masks: with the world in scalar registers (mn_query.hip's UNIFORM
// form) and the structs read as kernel arguments the kernel had 149 scalar spills, with only the world in LDS 79, as it stands none.
// The launch owns every pixel, so whole words leave with plain vector stores.
//
// mn_render_draw_kernel.  One WAVEFRONT per primitive (a stride loop over the primitives): the record is read at a wave-uniform address and planned
// once (mnr_plan: image range, clipped geometry, items per image); the (image, item) pairs -- the samples of a segment in each of its images, the
// box pixels of a disc in each of its images -- are dealt to the 64 lanes round robin, so a trail segment that goes into 200 frames and a disc that
// goes into one fill their wavefront alike.  Every write is an atomicMax on the pixel word: the picture does not depend on this mapping or on the
// order of arrival.  The kernels only READ the handle's arrays.
#include "mn_render_body.h"

#define MNR_BLOCK 256
#define MNR_TILE_W 64
#define MNR_TILE_H 4
#define MNR_MAX_BLOCKS 2048      // 8 workgroups per CU of a 256-CU device; more tiles than that: the stride loop

// one world as a workgroup holds it in LDS while it serves a tile of that world's image
struct MnrWorld {
    MnqCores C;
    double ox[MN_MAX_OBS], oy[MN_MAX_OBS], orad[MN_MAX_OBS];
    double start_x, start_y, goal_x, goal_y;
    int no, ok;
    __device__ __forceinline__ void obstacle(int k, double &x, double &y, double &r) const { x = ox[k]; y = oy[k]; r = orad[k]; }
};
static_assert(offsetof(MnqCores, cy) == 8 * MN_MAX_CORES && offsetof(MnqCores, cg) == 16 * MN_MAX_CORES, "the cores are filled as one [3][8] block");
static_assert(offsetof(MnrWorld, oy) - offsetof(MnrWorld, ox) == 8 * MN_MAX_OBS && offsetof(MnrWorld, orad) - offsetof(MnrWorld, ox) == 16 * MN_MAX_OBS &&
              offsetof(MnrWorld, goal_y) - offsetof(MnrWorld, start_x) == 24, "the obstacles are filled as one [3][10] block, start and goal as one [4]");
// the handle's table pointers and the launch's own, parked in LDS by the prologue: they are needed once per (workgroup, image) or once per pixel
struct MnrTables {
    const double *core[3], *obst[3], *pose[4];
    const int32_t *counts, *env_of;
    uint32_t *pixels;
    int n, npad, env0;
};
struct MnrFrame {
    MnDev P;
    MnrView V;
    mn_render_style S;
};
struct MnrLdsPalette {
    const uint32_t *pal;
    __device__ __forceinline__ uint32_t operator()(int level) const { return pal[level]; }
};

__global__ __launch_bounds__(MNR_BLOCK) void mn_render_worlds_kernel(const MnArrays A, const MnDev P, const int32_t *__restrict__ env_of, int env0,
                                                                     int n_images, const MnrView V, const mn_render_style S,
                                                                     uint32_t *__restrict__ pixels) {
    __shared__ MnrWorld w;
    __shared__ MnrTables tab;
    __shared__ MnrFrame fr;
    {      // the argument block's structs into LDS, one 32-bit word per lane and pass
        const uint32_t *ps = reinterpret_cast<const uint32_t *>(&S), *pv = reinterpret_cast<const uint32_t *>(&V), *pp = reinterpret_cast<const uint32_t *>(&P);
        for (unsigned k = threadIdx.x; k < sizeof(S) / 4; k += MNR_BLOCK) reinterpret_cast<uint32_t *>(&fr.S)[k] = ps[k];
        for (unsigned k = threadIdx.x; k < sizeof(V) / 4; k += MNR_BLOCK) reinterpret_cast<uint32_t *>(&fr.V)[k] = pv[k];
        for (unsigned k = threadIdx.x; k < sizeof(P) / 4; k += MNR_BLOCK) reinterpret_cast<uint32_t *>(&fr.P)[k] = pp[k];
    }
    if (threadIdx.x == MN_WAVE) {
        tab.core[0] = A.cx; tab.core[1] = A.cy; tab.core[2] = A.cg; tab.obst[0] = A.ox; tab.obst[1] = A.oy; tab.obst[2] = A.orad;
        tab.pose[0] = A.start_x; tab.pose[1] = A.start_y; tab.pose[2] = A.goal_x; tab.pose[3] = A.goal_y;
        tab.counts = A.counts; tab.n = A.n; tab.npad = A.npad; tab.env_of = env_of; tab.env0 = env0; tab.pixels = pixels;
    }
    __syncthreads();
    const MnrLdsPalette palette = {fr.S.palette};
    const int tiles_x = (V.W + MNR_TILE_W - 1) / MNR_TILE_W, tiles_y = (V.H + MNR_TILE_H - 1) / MNR_TILE_H;
    const int per_image = tiles_x * tiles_y, n_tiles = per_image * n_images;      // (at most one tile per pixel: below 2^31)
    const int lane_c = threadIdx.x & (MNR_TILE_W - 1), lane_r = threadIdx.x / MNR_TILE_W;
    int held = -1;      // the image whose world the LDS copy is (block-uniform)
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {      // (block-uniform trip count: the barriers below are met by all)
        const int img = tile / per_image, t = tile % per_image;
        if (img != held) {
            __syncthreads();      // the last tile's readers are done with the copy
            const int e = tab.env_of ? tab.env_of[img] : tab.env0;
            const bool ok = e >= 0 && e < tab.n;
            const int k = threadIdx.x;
            // lanes 0-23: core table k / 8, row k % 8; lanes 64-93: obstacle table, row; lanes 128-131: start and goal; lane 192: the counts
            if (ok && k < 3 * MN_MAX_CORES) (&w.C.cx[0])[k] = tab.core[k / MN_MAX_CORES][(size_t)(k % MN_MAX_CORES) * tab.npad + e];
            const int ko = k - MN_WAVE;
            if (ok && ko >= 0 && ko < 3 * MN_MAX_OBS) (&w.ox[0])[ko] = tab.obst[ko / MN_MAX_OBS][(size_t)(ko % MN_MAX_OBS) * tab.npad + e];
            const int kp = k - 2 * MN_WAVE;
            if (ok && kp >= 0 && kp < 4) (&w.start_x)[kp] = tab.pose[kp][e];
            if (k == 3 * MN_WAVE) {
                const int counts = ok ? tab.counts[e] : 0;
                w.C.nc = counts & 0xff; w.no = (counts >> 8) & 0xff; w.ok = ok;
            }
            held = img;
            __syncthreads();
        }
        const int c = (t % tiles_x) * MNR_TILE_W + lane_c, r = (t / tiles_x) * MNR_TILE_H + lane_r;
        if (c < fr.V.W && r < fr.V.H) {
            uint32_t word = fr.S.outside & 0xffffffu;
            if (w.ok) word = mnr_world_pixel(w.C, w, w.no, w.start_x, w.start_y, w.goal_x, w.goal_y, fr.P, fr.V, fr.S, palette, c, r);
            tab.pixels[((size_t)img * fr.V.H + r) * fr.V.W + c] = word;
        }
    }
}

struct MnrAtomicPut {
    uint32_t *image;      // of this lane's current item
    int W;
    uint32_t word;
    __device__ __forceinline__ void operator()(int c, int r) { atomicMax(image + (size_t)r * W + c, word); }
};

__global__ __launch_bounds__(MNR_BLOCK) void mn_render_draw_kernel(uint32_t *__restrict__ pixels, int n_images, const MnrView V,
                                                                   const mn_render_prim *__restrict__ prims, long long n_prims) {
    const int lane = threadIdx.x & (MN_WAVE - 1);
    const long long wave = (long long)blockIdx.x * (MNR_BLOCK / MN_WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / MN_WAVE);
    const long long n_waves = (long long)gridDim.x * (MNR_BLOCK / MN_WAVE);
    for (long long p = wave; p < n_prims; p += n_waves) {
        MnrPlan L;
        if (!mnr_plan(prims[p], V, n_images, L) || L.per_image <= 0) continue;
        const long long items = L.per_image * (L.i1 - L.i0 + 1);
        for (long long it = lane; it < items; it += MN_WAVE) {
            const int img = L.i0 + (int)(it / L.per_image);
            MnrAtomicPut put = {pixels + (size_t)img * V.H * V.W, V.W, L.word};
            mnr_item(L, V, it % L.per_image, put);
        }
    }
}

void mn_launch_render_worlds(const MnArrays &A, const MnDev &P, const int32_t *env_of, int env0, int n_images, int width, int height, const double view[4],
                             const mn_render_style &style, uint32_t *pixels, hipStream_t s) {
    const MnrView V = mnr_view(view, width, height);
    const long long tiles = (long long)((width + MNR_TILE_W - 1) / MNR_TILE_W) * ((height + MNR_TILE_H - 1) / MNR_TILE_H) * n_images;
    const long long cap = style.max_workgroups > 0 ? style.max_workgroups : MNR_MAX_BLOCKS;
    const dim3 grid((unsigned)(tiles < cap ? tiles : cap)), block(MNR_BLOCK);
    hipLaunchKernelGGL(mn_render_worlds_kernel, grid, block, 0, s, A, P, env_of, env0, n_images, V, style, pixels);
}

void mn_launch_render_draw(uint32_t *pixels, int n_images, int width, int height, const double view[4], const mn_render_prim *prims, int64_t n_prims,
                           hipStream_t s) {
    const MnrView V = mnr_view(view, width, height);
    const long long blocks = (n_prims + MNR_BLOCK / MN_WAVE - 1) / (MNR_BLOCK / MN_WAVE);
    const dim3 grid((unsigned)(blocks < MNR_MAX_BLOCKS ? blocks : MNR_MAX_BLOCKS)), block(MNR_BLOCK);
    hipLaunchKernelGGL(mn_render_draw_kernel, grid, block, 0, s, pixels, n_images, V, prims, (long long)n_prims);
}
