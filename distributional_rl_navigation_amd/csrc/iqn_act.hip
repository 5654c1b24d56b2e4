// iqn_act.hip -- fused IQN action-value kernel for gfx950 (MI355X).
//
// Replaces, for inference on a whole vector of environments, ObsEncoder.forward + the mean over the
// K = 32 quantile samples of ObsEncoder.get_qvals (thirdparty/IQN/model.py:141-191):
//     cos   = cos(tau * pi * [0..63])                                  (model.py:149-155)
//     x     = relu(cos @ W1^T + b1) * features                         (:177-181, Hadamard)
//     x     = relu(x @ W2^T + b2) ; x = relu(x @ W3^T + b3) ; q = x @ W4^T + b4   (:183-185)
//     Q     = mean over the K taus                                      (:188-191)
// The three linear observation encoders (:170-173, a block-diagonal 26 -> 208 map, <1 % of the FLOPs)
// run on the VALU inside the kernel (each lane computes 3-4 of the 208 features from the wave-uniform
// observation row and parks them in a per-wave LDS buffer), so the only inputs are the raw
// observations and the taus.  An optional epilogue does the
// argmax and the epsilon-greedy choice of IQNAgent.act (agent.py:199-203).
//
// Why a kernel: in eager PyTorch this path is ~95 % of a training vector step at 65 536 envs and is
// bound by elementwise traffic -- the [n*32, 208] activation is written and re-read five times
// (profiles/r01_full_loop_kernel_stats_v1.txt).  Here a wavefront owns one environment (32 tau rows)
// at a time and carries it through all four layers in registers; nothing but observations, taus and
// the 9 Q-values / the action touches HBM.
//
// The kernels live in three headers, one per family: iqn_act_exact.h (exact-f32 MFMA, variant 0), iqn_act_split.h (the same network on the
// f16 matrix pipe at float32 accuracy, variant 2: the default) and iqn_act_tiled.h (launch-shared taus with the environments in the MFMA
// columns).  This file is the host side: the kernel forms, the per-caller context, the one launch routine and the C ABI.  (The MFMA clock probe
// at the end, mfma_probe.h, is a measurement aid that shares the translation unit, nothing more.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>
#include <vector>

#include "marinenav_hip.h"
#include "mn_internal.h"
#include "iqn_actor_group.h"

#define MN_IQN_VARIANT_DEFAULT 2

namespace {

#include "iqn_act_common.h"
#include "iqn_act_exact.h"
#include "iqn_act_split.h"
#include "iqn_act_few.h"
#include "iqn_act_tiled.h"
#include "iqn_act_group.h"

// A kernel form = (kernel, dynamic LDS, workgroup size); the member of its family is set.  mn_iqn_create raises the LDS limit of every entry and
// launch_act launches the entry form_of picks with that entry's size, so the registered and the launched size of a form are one number.
using ExactKernel = decltype(&iqn_qvals_kernel<false>);
using SplitKernel = decltype(&sp::iqn_qvals_split_kernel<false>);
using TiledKernel = decltype(&sp::iqn_qvals_tiled_kernel);
struct Form {
    ExactKernel exact;
    SplitKernel split;
    TiledKernel tiled;
    int lds_floats, threads;
    const void *kernel() const { return exact ? (const void *)exact : split ? (const void *)split : (const void *)tiled; }
    size_t lds_bytes() const { return lds_floats * sizeof(float); }
};
enum { F_EXACT, F_EXACT_QUANT, F_SPLIT, F_SPLIT_LATE, F_SPLIT_ROWS, F_SPLIT_LATE_ROWS, F_SPLIT_QUANT, F_SHARED, F_SHARED_QUANT, F_TILED, N_FORMS };
const Form FORMS[N_FORMS] = {
    {iqn_qvals_kernel<false>, nullptr, nullptr, LDS_FLOATS, 512},
    {iqn_qvals_kernel<true>, nullptr, nullptr, LDS_FLOATS, 512},      // act_eval: the [n][32][9] quantile values as well
    {nullptr, sp::iqn_qvals_split_kernel<false>, nullptr, sp::LDS_ACT_FLOATS, 512},
    {nullptr, sp::iqn_qvals_split_kernel<false, false, sp::WAVES, true>, nullptr, sp::LDS_ACT_FLOATS, 512},      // late rows (mn_iqn_set_late_rows)
    {nullptr, sp::iqn_qvals_split_kernel<false, false, sp::WAVES, false, true>, nullptr, sp::LDS_ACT_FLOATS, 512},      // only the rows that do not explore (mn_iqn_set_greedy_rows)
    {nullptr, sp::iqn_qvals_split_kernel<false, false, sp::WAVES, true, true>, nullptr, sp::LDS_ACT_FLOATS, 512},       // ... with late rows among them
    {nullptr, sp::iqn_qvals_split_kernel<true>, nullptr, sp::LDS_FLOATS, 512},
    // launch-shared taus (12 waves per workgroup -- three per SIMD, the kernel needs 153 registers -- measured: 202-204 us against 203, no gain)
    {nullptr, sp::iqn_qvals_split_kernel<false, true, 8>, nullptr, sp::OFF_FB, 512},
    {nullptr, sp::iqn_qvals_split_kernel<true, true, 8>, nullptr, sp::OFF_FB, 512},
    {nullptr, nullptr, sp::iqn_qvals_tiled_kernel, sp::TL_FLOATS, 512},      // ... with the environments in the MFMA columns (iqn_act_tiled.h)
};

// NULL checks + fill of the 14 weight pointers of the C ABI
bool load_weights(const float *const *p, IqnWeights *w) {
    if (!p) return false;
    for (int i = 0; i < 14; ++i) if (!p[i]) return false;
    *w = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13]};
    return true;
}

}  // namespace

// Per-caller state of the act path: the permuted LDS weight image (cached between calls until the caller says the
// weights changed), the profiling events.  One context per agent / per stream: two contexts never share a buffer, so
// agents acting on different streams of one device cannot race on the image.
struct mn_iqn_ctx {
    int device = -1;
    int n_cu = 0;
    float *packed = nullptr;       // weight image of the exact-f32 16x16x4 kernel (variant 0)
    uint32_t *packed_sp = nullptr; // weight image of the split-f16 kernel (iqn_act_split.h)
    float *consts_sp = nullptr;    // its scale / bound constants
    float *h1_sp = nullptr;        // the launch's layer-1 constant [32 taus x 208] of the shared-tau kernels (mn_iqn_set_tau_mode) + 32 block maxima
    uint32_t *timg = nullptr;      // tiled shared-tau kernel (iqn_act_tiled.h): T = W2 h1 as hi / lo f16 pairs, and its auxiliary float block
    float *taux = nullptr;
    // the buffers above with their element counts: the one list that create, its failure path and destroy walk
    template <class Fn> void each_buffer(Fn f) {
        f(packed, OFF_FB); f(packed_sp, sp::OFF_FB); f(consts_sp, sp::N_CONST_BUF); f(h1_sp, sp::H1_FLOATS + 32); f(timg, sp::T_WORDS); f(taux, sp::TA_FLOATS);
    }
    int tau_mode = 0;              // 0 = every environment its own 32 taus (the reference's per-call draw), 1 = one set of 32 per launch
    bool dirty = true, dirty_sp = true;
    int variant = MN_IQN_VARIANT_DEFAULT;   // mn_iqn_set_variant
    int max_blocks = 0;                     // mn_iqn_set_grid: 0 = one persistent workgroup per CU
    sp::LateRows late = {};                 // mn_iqn_set_late_rows: consumed by the next launch
    uint32_t *late_status = nullptr;        // waits of late rows that ran out (device word)
    volatile uint32_t *late_status_host = nullptr;      // ... and the host-mapped copy the kernel keeps of it (mn_iqn_late_timeouts_peek: no synchronisation)
    uint32_t *late_status_host_dev = nullptr;
    uint64_t late_bound_ticks = sp::LATE_BOUND_TICKS;    // mn_iqn_set_late_bound_ms
    std::vector<hipEvent_t> ev;
    int prof_max = 0, prof_n = 0;
    uint32_t *rollout_words = nullptr;      // mn_rollout_iqn: its launch's ticket and longest episode (zero between launches)
    bool greedy_rows = true;                // mn_iqn_set_greedy_rows
    uint32_t *rows_buf = nullptr;           // GreedyRows of the act launches: 4 words, then the list [rows_cap]
    int rows_cap = 0;
    int few_rows_max = MN_IQN_FEW_ROWS_MAX_DEFAULT;      // mn_iqn_set_few_rows_max
    int64_t few_launches = 0;               // act launches that ran as the few-rows kernel (mn_iqn_few_rows_launches)
};

extern "C" int mn_iqn_set_grid(mn_iqn_ctx *c, int32_t max_workgroups) {
    if (!c || max_workgroups < 0) return MN_ERR_INVALID;
    c->max_blocks = max_workgroups;
    return MN_OK;
}

extern "C" int mn_iqn_create(mn_iqn_ctx **out) {
    if (!out) return MN_ERR_INVALID;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return MN_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return MN_ERR_HIP;
    // per-device function attribute; setting it again for another context is harmless and has no shared host state
    for (const Form &f : FORMS)
        if (hipFuncSetAttribute(f.kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds_bytes()) != hipSuccess) return MN_ERR_HIP;
    mn_iqn_ctx *c = new mn_iqn_ctx();
    c->device = dev;
    c->n_cu = prop.multiProcessorCount;
    bool ok = true;
    c->each_buffer([&](auto *&p, size_t count) { ok = ok && hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(*p)) == hipSuccess; });
    if (!ok || hipMemset(c->consts_sp, 0, sp::N_CONST_BUF * sizeof(float)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        c->each_buffer([](auto *p, size_t) { (void)hipFree(p); });
        delete c;
        return MN_ERR_ALLOC;
    }
    *out = c;
    return MN_OK;
}

extern "C" int mn_iqn_destroy(mn_iqn_ctx *c) {
    if (!c) return MN_ERR_INVALID;
    int cur = -1;
    const bool moved = hipGetDevice(&cur) == hipSuccess && cur != c->device;
    if (moved) (void)hipSetDevice(c->device);
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    c->each_buffer([](auto *p, size_t) { (void)hipFree(p); });
    (void)hipFree(c->late_status);
    (void)hipFree(c->rollout_words);
    (void)hipFree(c->rows_buf);
    if (c->late_status_host) (void)hipHostFree((void *)c->late_status_host);
    if (moved) (void)hipSetDevice(cur);
    delete c;
    return MN_OK;
}

extern "C" int mn_iqn_weights_changed(mn_iqn_ctx *c) {
    if (!c) return MN_ERR_INVALID;
    c->dirty = true;
    c->dirty_sp = true;
    return MN_OK;
}

extern "C" int mn_iqn_set_variant(mn_iqn_ctx *c, int32_t variant) {
    if (!c || (variant != 0 && variant != 2)) return MN_ERR_INVALID;      // (1 and 3 were the 32x32 re-layouts of the two kernels: measured slower, removed in round 6)
    c->variant = variant;
    return MN_OK;
}

extern "C" int mn_iqn_set_greedy_rows(mn_iqn_ctx *c, int32_t on) {
    if (!c) return MN_ERR_INVALID;
    c->greedy_rows = on != 0;
    return MN_OK;
}

// The listed-rows launch (F_SPLIT_ROWS) runs as sp::iqn_act_few_kernel (iqn_act_few.h: no LDS image, two wavefronts per row) while the list is expected
// to hold at most `rows` rows, (1 - eps) n: negative = never, 0x7fffffff = always.  Same actions, draws and call counter either way.
extern "C" int mn_iqn_set_few_rows_max(mn_iqn_ctx *c, int32_t rows) {
    if (!c) return MN_ERR_INVALID;
    c->few_rows_max = rows;
    return MN_OK;
}

// Act launches of this context that ran as the few-rows kernel so far (test hook: which kernel a call took is not visible in its results)
extern "C" int mn_iqn_few_rows_launches(mn_iqn_ctx *c, int64_t *out) {
    if (!c || !out) return MN_ERR_INVALID;
    *out = c->few_launches;
    return MN_OK;
}

// The context's GreedyRows for a launch of `n` rows: allocated, or grown, on the first launch of that size (words zero: both count slots armed)
static int greedy_rows_buffer(mn_iqn_ctx *c, int n, GreedyRows *out) {
    if (n > c->rows_cap) {
        uint32_t *buf = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&buf), (4 + (size_t)n) * sizeof(uint32_t)) != hipSuccess) return MN_ERR_ALLOC;
        if (hipMemset(buf, 0, 4 * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipFree(buf); return MN_ERR_HIP; }
        (void)hipFree(c->rows_buf);      // (behind the synchronisation: no launch still reads it)
        c->rows_buf = buf;
        c->rows_cap = n;
    }
    *out = GreedyRows{reinterpret_cast<int32_t *>(c->rows_buf + 4), c->rows_buf};
    return MN_OK;
}

// The rows the last act launch with listed rows evaluated (test hook): *count_out of them, the first min(count, cap) indices in list_host (any order).
// Synchronises `stream`.  Count 0 and MN_OK before the first such launch.
extern "C" int mn_iqn_last_greedy_rows(mn_iqn_ctx *c, void *stream, int32_t *list_host, int32_t cap, int32_t *count_out) {
    if (!c || !count_out || cap < 0 || (cap > 0 && !list_host)) return MN_ERR_INVALID;
    *count_out = 0;
    if (!c->rows_buf) return MN_OK;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return MN_ERR_HIP;
    uint32_t w[4];
    if (hipMemcpy(w, c->rows_buf, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return MN_ERR_HIP;
    const uint32_t count = w[w[2] & 1u];      // words[2]: the slot the last preparation launch counted in
    if (count > (uint32_t)c->rows_cap) return MN_ERR_HIP;
    *count_out = (int32_t)count;
    const uint32_t k = count < (uint32_t)cap ? count : (uint32_t)cap;
    if (k && hipMemcpy(list_host, c->rows_buf + 4, k * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return MN_ERR_HIP;
    return MN_OK;
}

extern "C" int mn_iqn_set_tau_mode(mn_iqn_ctx *c, int32_t mode) {
    if (!c || mode < 0 || mode > 3) return MN_ERR_INVALID;
    c->tau_mode = mode;
    return MN_OK;
}

extern "C" int mn_iqn_profile_begin(mn_iqn_ctx *c, int32_t max_launches) {
    if (!c || max_launches < 0 || max_launches > 65536) return MN_ERR_INVALID;
    while ((int)c->ev.size() < 2 * max_launches) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return MN_ERR_HIP;
        c->ev.push_back(e);
    }
    c->prof_max = max_launches;
    c->prof_n = 0;
    return MN_OK;
}

extern "C" int mn_iqn_profile_end(mn_iqn_ctx *c, void *stream, double *mean_ms, int32_t *launches) {
    if (!c) return MN_ERR_INVALID;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return MN_ERR_HIP;
    double sum = 0.0;
    for (int i = 0; i < c->prof_n; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev[2 * i], c->ev[2 * i + 1]) != hipSuccess) return MN_ERR_HIP;
        sum += ms;
    }
    if (mean_ms) *mean_ms = c->prof_n ? sum / c->prof_n : 0.0;
    if (launches) *launches = c->prof_n;
    c->prof_max = 0;
    c->prof_n = 0;
    return MN_OK;
}

// Workgroups of the wave-per-environment forms: eight environments per workgroup pass, capped by mn_iqn_set_grid or at one persistent workgroup per CU
static int act_grid(const mn_iqn_ctx *c, int n) {
    const int blocks = (n + 7) / 8, cap = c->max_blocks > 0 ? c->max_blocks : c->n_cu;
    return blocks < cap ? blocks : cap;
}

// Whether a launch of `n` rows at `eps` in form `f` runs as the few-rows kernel (mn_iqn_set_few_rows_max): the rule reads the EXPECTED length of the list, as
// mn_reset_placement does -- the host does not know the count
static bool few_rows(const mn_iqn_ctx *c, const Form &f, int n, float eps) {
    if (&f != &FORMS[F_SPLIT_ROWS] || c->few_rows_max < 0) return false;
    return (1.0 - (eps < 1.f ? (double)eps : 1.0)) * (double)n <= (double)c->few_rows_max;
}

// Its workgroups, one list position each at a time: as many as the threshold lets the list be long, capped like act_grid (a longer list loops)
static int few_grid(const mn_iqn_ctx *c, int n) {
    const int cap = c->max_blocks > 0 ? c->max_blocks : c->n_cu, want = c->few_rows_max < 1 ? 1 : c->few_rows_max;
    const int blocks = want < cap ? want : cap;
    return blocks < n ? blocks : n;
}

// Blocks of 256 threads that make a launch's `items` draws beside the pack blocks of a prep kernel
static int draw_blocks(const mn_iqn_ctx *c, long items) {
    const long blocks = (items + 255) / 256;
    return blocks < 8L * c->n_cu ? (int)blocks : 8 * c->n_cu;
}

// The acting kernel that takes late rows: split-f16, per-environment taus, no quantile capture, at most 64 rows per wavefront.
static bool late_rows_supported(const mn_iqn_ctx *c, int n, bool quantiles) {
    if (c->variant != 2 || c->tau_mode != 0 || quantiles || n <= 0) return false;
    return (long)n <= 64L * 8L * act_grid(c, n);
}

// Rows of the next act launch whose observation is still being written by a reset launch on another stream (mn_reset_done_async):
// `mask_dev` [n] (the step's done flags), `flags_dev` [n] / `tick` from mn_reset_done_async.  Returns MN_OK if the next launch of `n` rows will
// take them (then launch it with nothing in between), 1 if this context's current form cannot -- the caller then joins the reset (mn_reset_join) first.
extern "C" int mn_iqn_set_late_rows(mn_iqn_ctx *c, const uint8_t *mask_dev, const uint32_t *flags_dev, uint32_t tick, int32_t n) {
    if (!c) return MN_ERR_INVALID;
    c->late = sp::LateRows{};
    if (!mask_dev && !flags_dev) return MN_OK;      // clear
    if (!mask_dev || !flags_dev) return MN_ERR_INVALID;
    if (!late_rows_supported(c, n, false)) return 1;
    if (!c->late_status) {      // (all or nothing: the context only keeps the words once every allocation has succeeded)
        uint32_t *st = nullptr;
        void *hp = nullptr, *hd = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&st), sizeof(uint32_t)) != hipSuccess) return MN_ERR_ALLOC;
        if (hipMemset(st, 0, sizeof(uint32_t)) != hipSuccess || hipHostMalloc(&hp, sizeof(uint32_t), hipHostMallocMapped) != hipSuccess) { (void)hipFree(st); return MN_ERR_ALLOC; }
        *(volatile uint32_t *)hp = 0u;
        if (hipHostGetDevicePointer(&hd, hp, 0) != hipSuccess) { (void)hipFree(st); (void)hipHostFree(hp); return MN_ERR_HIP; }
        c->late_status = st; c->late_status_host = (volatile uint32_t *)hp; c->late_status_host_dev = (uint32_t *)hd;
    }
    c->late = sp::LateRows{mask_dev, flags_dev, tick, c->late_status, c->late_status_host_dev, c->late_bound_ticks};
    return MN_OK;
}

// Waits for a late row that ran out since the context was made (0 in a healthy run; anything else: actions were computed on unfinished observations).
extern "C" int mn_iqn_late_timeouts(mn_iqn_ctx *c, void *stream, uint32_t *out) {
    if (!c || !out) return MN_ERR_INVALID;
    *out = 0;
    if (!c->late_status) return MN_OK;
    if (hipMemcpyAsync(out, c->late_status, sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) return MN_ERR_HIP;
    return hipStreamSynchronize((hipStream_t)stream) == hipSuccess ? MN_OK : MN_ERR_HIP;
}

// The same count as the launches executed so far have left it in a host-mapped word: no synchronisation, so a training loop can look every few
// vector steps (a launch still in flight is not counted yet).
extern "C" int mn_iqn_late_timeouts_peek(mn_iqn_ctx *c, uint32_t *out) {
    if (!c || !out) return MN_ERR_INVALID;
    *out = c->late_status_host ? *c->late_status_host : 0u;
    return MN_OK;
}

// Bound of a late row's wait in milliseconds (default 500; tests use a short one).  Applies to launches armed after the call.
extern "C" int mn_iqn_set_late_bound_ms(mn_iqn_ctx *c, double ms) {
    if (!c || !(ms > 0.0) || ms > 60000.0) return MN_ERR_INVALID;
    c->late_bound_ticks = (uint64_t)(ms * 1.0e5);      // 100 MHz counter
    return MN_OK;
}

// The form a launch of `n` rows runs in (variants, mn_iqn_set_variant: 0 = exact-f32 16x16x4 kernel, 2 = split-f16 kernel; tau modes, mn_iqn_set_tau_mode:
// shared taus run with the environments in the MFMA columns from sp::TILED_MIN_ENVS rows, in mode 3 always, and never with quantiles).  `rows`: the launch
// writes nothing but actions and its preparation launch has settled the exploring rows (launch_act), so only the listed rows are evaluated.
static const Form &form_of(const mn_iqn_ctx *c, int n, bool quantiles, bool late, bool rows) {
    if (c->tau_mode != 0) {
        if (!quantiles && ((c->tau_mode == 1 && n >= sp::TILED_MIN_ENVS) || c->tau_mode == 3)) return FORMS[F_TILED];
        return FORMS[quantiles ? F_SHARED_QUANT : F_SHARED];
    }
    if (c->variant != 2) return FORMS[quantiles ? F_EXACT_QUANT : F_EXACT];
    if (rows && !quantiles) return FORMS[late ? F_SPLIT_LATE_ROWS : F_SPLIT_ROWS];
    return FORMS[quantiles ? F_SPLIT_QUANT : late ? F_SPLIT_LATE : F_SPLIT];
}

// Begins the rebuild of the variant's weight image if it is stale (mn_iqn_weights_changed): returns the block count of its pack, 0 for a cached image, with
// the split image's constants enqueued.  The caller enqueues the pack next -- pack_image, or a prep kernel that packs in its first blocks.
static int begin_pack(mn_iqn_ctx *c, const IqnWeights &w, hipStream_t s) {
    bool &stale = c->variant == 2 ? c->dirty_sp : c->dirty;
    if (!stale) return 0;
    stale = false;
    if (c->variant != 2) return PACK_BLOCKS;
    hipLaunchKernelGGL(sp::iqn_split_consts_kernel, dim3(sp::CONST_BLOCKS), dim3(256), 0, s, w, c->consts_sp);
    return sp::PACK_BLOCKS;
}

static void pack_image(mn_iqn_ctx *c, const IqnWeights &w, hipStream_t s) {
    if (c->variant == 2) hipLaunchKernelGGL(sp::iqn_split_pack_kernel, dim3(sp::PACK_BLOCKS), dim3(256), 0, s, w, (const float *)c->consts_sp, c->packed_sp);
    else hipLaunchKernelGGL(iqn_pack_kernel, dim3(PACK_BLOCKS), dim3(256), 0, s, w, c->packed);
}

static int launch_act(mn_iqn_ctx *c, const float *obs_dev, const float *taus_dev, const float *const *weights, float *qvals_dev,
                      const float *explore_u_dev, float eps, int32_t *actions_dev, float *quantiles_dev, int32_t n,
                      int32_t num_taus, uint64_t *rng_state_dev, float *draws_dev, const float *cvar_row_dev, float cvar,
                      void *stream, mn_handle *env = nullptr) {
    // ---- prologue: arguments, the launch's form, its armed late rows
    IqnWeights w;
    if (!c || !obs_dev || !load_weights(weights, &w) || (!qvals_dev && !actions_dev && !quantiles_dev)) return MN_ERR_INVALID;
    if (rng_state_dev ? !draws_dev : !taus_dev) return MN_ERR_INVALID;
    if (rng_state_dev && (long)n * (K_TAUS + 1) >= (1L << 32)) return MN_ERR_INVALID;   // 32-bit draw index
    if (n <= 0 || num_taus != K_TAUS) return MN_ERR_INVALID;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != c->device) return MN_ERR_INVALID;   // context lives on another device
    hipStream_t s = (hipStream_t)stream;
    // late rows (mn_iqn_set_late_rows) belong to THIS launch only; a form that cannot honour them must never see them (the caller joined the reset instead)
    const sp::LateRows late = c->late;
    c->late = sp::LateRows{};
    if (late.mask && !late_rows_supported(c, n, quantiles_dev != nullptr)) return MN_ERR_INVALID;
    // Launch-shared taus: ONE set of 32 quantile fractions for every environment of the launch (iqn_act_split.h, stage_sh).  Only the
    // split-f16 kernel has this form; per-row CVaR (adaptive policies) needs per-environment taus.
    const bool shared = c->tau_mode != 0, rng = rng_state_dev != nullptr;
    if (shared && (c->variant != 2 || cvar_row_dev)) return MN_ERR_INVALID;
    // Only the rows that do not explore (mn_iqn_set_greedy_rows): the library's own draws, per-row taus, nothing asked for but the actions.  Q values and
    // quantiles are read by the caller for every row, and injected uniforms (mn_iqn_act) have no preparation launch to settle them in.
    const bool listed = c->greedy_rows && rng && !shared && c->variant == 2 && actions_dev && !qvals_dev && !quantiles_dev && eps > 0.f;
    GreedyRows rows = {};
    if (listed) {
        const int rc = greedy_rows_buffer(c, n, &rows);
        if (rc) return rc;
    }
    const Form &f = form_of(c, n, quantiles_dev != nullptr, late.mask != nullptr, listed);
    // `env` (mn_iqn_act_rng_env) may owe the reset of its last step's finished envs: the split form's preparation launch takes it along (mn_prep_reset.hip);
    // any other form reads its observations behind a plain reset launch
    const bool fusable = f.split && rng && !shared;
    if (env && !fusable) {
        const int rc = mn_owed_reset_settle(env, s);
        if (rc) return rc;
    }
    const bool prof = c->prof_n < c->prof_max;
    if (prof) (void)hipEventRecord(c->ev[2 * c->prof_n], s);

    // ---- prepare: the weight image if it is stale and the launch's draws, in one launch where both are due
    const int pack_blocks = begin_pack(c, w, s);
    if (shared) {      // (packs, draws the 32 taus and the n exploration uniforms, builds the layer-1 constant)
        const int rng_blocks = rng ? draw_blocks(c, (long)n + K_TAUS) : 0;
        hipLaunchKernelGGL(sp::iqn_shared_prep_kernel, dim3(pack_blocks + sp::H1_BLOCKS + rng_blocks), dim3(256), 0, s, w, (const float *)c->consts_sp,
                           c->packed_sp, (const uint64_t *)rng_state_dev, draws_dev, n, rng ? nullptr : taus_dev, cvar, pack_blocks, c->h1_sp);
        if (rng) explore_u_dev = eps > 0.f ? draws_dev + K_TAUS : nullptr;
        taus_dev = nullptr;
        if (f.tiled)      // large batch: the MFMA columns are environments (iqn_act_tiled.h): T = W2 h1 built once, 32 environments per wavefront
            hipLaunchKernelGGL(sp::iqn_tiled_prep_kernel, dim3(sp::T_PREP_BLOCKS + sp::TA_PREP_BLOCKS), dim3(256), 0, s, w, (const float *)c->consts_sp,
                               (const float *)c->h1_sp, c->timg, c->taux);
    } else if (rng) {      // (n x 32 taus and n exploration uniforms, as float4 groups)
        const int rng_blocks = draw_blocks(c, ((long)n * (K_TAUS + 1) + 3) / 4);
        MnOwedReset owed;
        if (fusable && env && mn_owed_reset_take(env, s, &owed))
            mn_launch_prep_reset(owed, MnPrepLaunch{weights, c->consts_sp, c->packed_sp, pack_blocks != 0, rng_state_dev, draws_dev, n, cvar_row_dev, cvar, eps,
                                                    listed ? actions_dev : nullptr, rows.list, rows.words, 32 * c->n_cu}, s);
        else if (f.split)
            hipLaunchKernelGGL(sp::iqn_split_prep_kernel, dim3(pack_blocks + rng_blocks), dim3(256), 0, s, w, (const float *)c->consts_sp,
                               c->packed_sp, (const uint64_t *)rng_state_dev, draws_dev, n, cvar_row_dev, cvar, pack_blocks, eps, listed ? actions_dev : nullptr,
                               rows);
        else
            hipLaunchKernelGGL(iqn_prep_kernel, dim3(pack_blocks + rng_blocks), dim3(256), 0, s, w, c->packed,
                               (const uint64_t *)rng_state_dev, draws_dev, n, cvar_row_dev, cvar, pack_blocks);
        taus_dev = draws_dev;
        explore_u_dev = eps > 0.f ? draws_dev + (size_t)n * K_TAUS : nullptr;
    } else if (pack_blocks) {
        pack_image(c, w, s);
    }

    // ---- launch
    const dim3 grid(act_grid(c, n)), block(f.threads);
    if (few_rows(c, f, n, eps)) {
        ++c->few_launches;
        hipLaunchKernelGGL(sp::iqn_act_few_kernel, dim3(few_grid(c, n)), dim3(64 * sp::FEW_WAVES), 0, s, obs_dev, taus_dev, (const uint32_t *)c->packed_sp, actions_dev,
                           n, rng_state_dev, rows);
    } else if (f.tiled)
        hipLaunchKernelGGL(f.tiled, dim3((n + 255) / 256), block, f.lds_bytes(), s, obs_dev, (const uint32_t *)c->packed_sp, (const uint32_t *)c->timg,
                           (const float *)c->taux, qvals_dev, explore_u_dev, eps, actions_dev, n, rng_state_dev);
    else if (f.split)
        hipLaunchKernelGGL(f.split, grid, block, f.lds_bytes(), s, obs_dev, taus_dev, (const uint32_t *)c->packed_sp, qvals_dev, explore_u_dev, eps,
                           actions_dev, n, rng_state_dev, quantiles_dev, shared ? (const float *)c->h1_sp : nullptr, late, rows);
    else
        hipLaunchKernelGGL(f.exact, grid, block, f.lds_bytes(), s, obs_dev, taus_dev, (const float *)c->packed, qvals_dev, explore_u_dev, eps,
                           actions_dev, n, rng_state_dev, quantiles_dev);

    // ---- epilogue
    if (prof) { (void)hipEventRecord(c->ev[2 * c->prof_n + 1], s); ++c->prof_n; }
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

extern "C" int mn_iqn_refresh(mn_iqn_ctx *c, const float *const *weights, void *stream) {
    IqnWeights w;
    if (!c || !load_weights(weights, &w)) return MN_ERR_INVALID;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != c->device) return MN_ERR_INVALID;
    if (begin_pack(c, w, (hipStream_t)stream)) pack_image(c, w, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

// What mn_rollout_iqn (mn_capi.hip) needs of a context: the split-f16 weight image, rebuilt first if stale (as mn_iqn_refresh, which also checks
// `weights`), and two device words for its launch.  MN_ERR_INVALID for the forms the rollout does not reproduce: the exact-f32 variant, launch-shared taus.
int mn_iqn_rollout_image(mn_iqn_ctx *c, const float *const *weights, hipStream_t s, const uint32_t **image, uint32_t **words) {
    if (!c || !weights || !image || !words || c->variant != 2 || c->tau_mode != 0) return MN_ERR_INVALID;
    if (!c->rollout_words) {
        uint32_t *w = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&w), 2 * sizeof(uint32_t)) != hipSuccess) return MN_ERR_ALLOC;
        if (hipMemset(w, 0, 2 * sizeof(uint32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipFree(w); return MN_ERR_HIP; }
        c->rollout_words = w;
    }
    const int rc = mn_iqn_refresh(c, weights, (void *)s);
    if (rc) return rc;
    *image = c->packed_sp;
    *words = c->rollout_words;
    return MN_OK;
}

extern "C" int32_t mn_iqn_image_floats(void) { return sp::ACT_IMG_FLOATS; }

// A copy of the acting image for mn_rollout_iqn_groups: the same image, under the same refusals, as mn_iqn_rollout_image hands to mn_rollout_iqn
extern "C" int mn_iqn_export_image(mn_iqn_ctx *c, const float *const *weights, uint32_t *image_out_dev, void *stream) {
    if (!c || !weights || !image_out_dev || c->variant != 2 || c->tau_mode != 0) return MN_ERR_INVALID;
    const int rc = mn_iqn_refresh(c, weights, stream);
    if (rc) return rc;
    if (hipMemcpyAsync(image_out_dev, c->packed_sp, sp::ACT_IMG_FLOATS * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
        return MN_ERR_HIP;
    return MN_OK;
}

extern "C" int mn_iqn_act(mn_iqn_ctx *c, const float *obs_dev, const float *taus_dev, const float *const *weights,
                          float *qvals_dev, const float *explore_u_dev, float eps, int32_t *actions_dev,
                          float *quantiles_dev, int32_t n, int32_t num_taus, void *stream) {
    return launch_act(c, obs_dev, taus_dev, weights, qvals_dev, explore_u_dev, eps, actions_dev, quantiles_dev, n, num_taus,
                      nullptr, nullptr, nullptr, 1.0f, stream);
}

extern "C" int mn_iqn_act_rng(mn_iqn_ctx *c, const float *obs_dev, const float *const *weights, uint64_t *rng_state_dev,
                              float *draws_dev, const float *cvar_row_dev, float cvar, float eps, int32_t *actions_dev,
                              float *qvals_dev, float *quantiles_dev, int32_t n, int32_t num_taus, void *stream) {
    if (!rng_state_dev) return MN_ERR_INVALID;
    return launch_act(c, obs_dev, nullptr, weights, qvals_dev, nullptr, eps, actions_dev, quantiles_dev, n, num_taus,
                      rng_state_dev, draws_dev, cvar_row_dev, cvar, stream);
}

extern "C" int mn_iqn_act_rng_env(mn_iqn_ctx *c, mn_handle *env, const float *obs_dev, const float *const *weights, uint64_t *rng_state_dev,
                                  float *draws_dev, const float *cvar_row_dev, float cvar, float eps, int32_t *actions_dev,
                                  float *qvals_dev, float *quantiles_dev, int32_t n, int32_t num_taus, void *stream) {
    if (!rng_state_dev) return MN_ERR_INVALID;
    return launch_act(c, obs_dev, nullptr, weights, qvals_dev, nullptr, eps, actions_dev, quantiles_dev, n, num_taus,
                      rng_state_dev, draws_dev, cvar_row_dev, cvar, stream, env);
}

// ---- many actors per launch (mn_iqn_actor_group_*; kernels: iqn_act_group.h; the append: replay.hip) -------------------------------------------------------
static bool extents_overlap(const void *p, size_t np, const void *q, size_t nq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + nq && b < a + np;
}

extern "C" int mn_iqn_actor_group_create(const mn_iqn_actor *actors_host, int32_t n_actors, int32_t rows_per_group, mn_iqn_actor_group **out) {
    if (!out) return MN_ERR_INVALID;
    *out = nullptr;
    if (!actors_host || n_actors < 1 || n_actors > MN_IQN_MAX_ACTORS || rows_per_group < 1) return MN_ERR_INVALID;
    if ((long)rows_per_group * (K_TAUS + 1) >= (1L << 32)) return MN_ERR_INVALID;      // 32-bit draw index, as a single call
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return MN_ERR_NO_DEVICE;
    const size_t draws_bytes = (size_t)rows_per_group * (K_TAUS + 1) * sizeof(float);
    bool rings = true;
    for (int g = 0; g < n_actors; ++g) {
        const mn_iqn_actor &a = actors_host[g];
        IqnWeights w;
        if (!a.ctx || !load_weights(a.weights, &w) || !a.rng_state || !a.draws) return MN_ERR_INVALID;
        if (a.ctx->device != dev || a.ctx->variant != 2 || a.ctx->tau_mode != 0) return MN_ERR_INVALID;
        const void *ring[5] = {a.ring_states, a.ring_next_states, a.ring_actions, a.ring_rewards, a.ring_dones};
        int given = 0;
        for (const void *p : ring) given += p != nullptr;
        if (given != 0 && given != 5) return MN_ERR_INVALID;
        rings = rings && given == 5;
        // actors that alias would race silently: nothing one actor writes may be what another writes
        for (int h = 0; h < g; ++h) {
            const mn_iqn_actor &b = actors_host[h];
            if (a.ctx == b.ctx || extents_overlap(a.draws, draws_bytes, b.draws, draws_bytes) ||
                extents_overlap(a.rng_state, 2 * sizeof(uint64_t), b.rng_state, 2 * sizeof(uint64_t)))
                return MN_ERR_INVALID;
            const void *other[5] = {b.ring_states, b.ring_next_states, b.ring_actions, b.ring_rewards, b.ring_dones};
            for (const void *p : ring)
                for (const void *q : other)
                    if (p && p == q) return MN_ERR_INVALID;
        }
    }
    if (!rings)      // (a group that only ever acts has no ring at all)
        for (int g = 0; g < n_actors; ++g)
            if (actors_host[g].ring_states) return MN_ERR_INVALID;
    // ---- the device from here on: the grouped kernels' LDS limit, every context's greedy-row buffer, the table
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return MN_ERR_HIP;
    for (const void *k : {(const void *)sp::iqn_group_act_kernel<false>, (const void *)sp::iqn_group_act_kernel<true>})
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sp::LDS_ACT_FLOATS * sizeof(float))) != hipSuccess) return MN_ERR_HIP;
    mn_iqn_actor_group *grp = new mn_iqn_actor_group{};
    grp->n_groups = n_actors; grp->rows = rows_per_group; grp->device = dev; grp->n_cu = prop.multiProcessorCount; grp->rings = rings;
    std::vector<IqnActorRow> table(n_actors);
    for (int g = 0; g < n_actors; ++g) {
        const mn_iqn_actor &a = actors_host[g];
        GreedyRows rows;
        const int rc = greedy_rows_buffer(a.ctx, rows_per_group, &rows);
        if (rc) { delete grp; return rc; }
        grp->ctx[g] = a.ctx;
        grp->rows_buf[g] = a.ctx->rows_buf;
        IqnActorRow &r = table[g];
        for (int i = 0; i < 14; ++i) r.weights[i] = a.weights[i];
        r.consts = a.ctx->consts_sp; r.packed = a.ctx->packed_sp; r.rng_state = a.rng_state; r.draws = a.draws; r.rows_buf = a.ctx->rows_buf;
        r.ring_states = a.ring_states; r.ring_next_states = a.ring_next_states; r.ring_actions = a.ring_actions;
        r.ring_rewards = a.ring_rewards; r.ring_dones = a.ring_dones;
    }
    if (hipMalloc(reinterpret_cast<void **>(&grp->table_dev), sizeof(IqnActorRow) * n_actors) != hipSuccess ||
        hipMemcpy(grp->table_dev, table.data(), sizeof(IqnActorRow) * n_actors, hipMemcpyHostToDevice) != hipSuccess) {
        if (grp->table_dev) (void)hipFree(grp->table_dev);
        delete grp;
        return MN_ERR_HIP;
    }
    *out = grp;
    return MN_OK;
}

extern "C" int mn_iqn_actor_group_destroy(mn_iqn_actor_group *g) {
    if (!g) return MN_ERR_INVALID;
    const hipError_t e = hipFree(g->table_dev);
    delete g;
    return e == hipSuccess ? MN_OK : MN_ERR_HIP;
}

// Workgroups per group of the grouped act launch.  Every workgroup that has a row copies the 154-KB image into LDS, one workgroup per CU at a time: G x
// act_grid(n) workgroups can be several rounds of CUs that each pay that copy again, so a group gets its share of the CUs (results do not depend on it).
// mn_iqn_set_grid on the FIRST actor's context replaces the share by its own cap (measurements: scripts/iqn_group_collect_bench.py).
static int group_act_grid(const mn_iqn_actor_group *g) {
    const int blocks = (g->rows + 7) / 8, share = g->n_cu / g->n_groups > 1 ? g->n_cu / g->n_groups : 1;
    const int cap = g->ctx[0]->max_blocks > 0 ? g->ctx[0]->max_blocks : share;
    return blocks < cap ? blocks : cap;
}

extern "C" int mn_iqn_actor_group_act(mn_iqn_actor_group *g, const float *obs_dev, float cvar, float eps, int32_t *actions_dev, void *stream) {
    if (!g || !obs_dev || !actions_dev) return MN_ERR_INVALID;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != g->device) return MN_ERR_INVALID;
    const int G = g->n_groups, n = g->rows;
    for (int i = 0; i < G; ++i) {      // what a context's setters may have changed since the group was made
        const mn_iqn_ctx *c = g->ctx[i];
        if (c->variant != 2 || c->tau_mode != 0 || c->late.mask || c->greedy_rows != g->ctx[0]->greedy_rows || c->rows_buf != g->rows_buf[i]) return MN_ERR_INVALID;
    }
    const bool listed = g->ctx[0]->greedy_rows && eps > 0.f;
    uint64_t stale = 0;
    for (int i = 0; i < G; ++i)
        if (g->ctx[i]->dirty_sp) { stale |= 1ull << i; g->ctx[i]->dirty_sp = false; }
    hipStream_t s = (hipStream_t)stream;
    const IqnActorRow *table = g->table_dev;
    if (stale) hipLaunchKernelGGL(sp::iqn_group_consts_kernel, dim3(sp::CONST_BLOCKS, G), dim3(256), 0, s, table, stale);
    const int pack_blocks = stale ? sp::PACK_BLOCKS : 0, rng_blocks = draw_blocks(g->ctx[0], ((long)n * (K_TAUS + 1) + 3) / 4);
    hipLaunchKernelGGL(sp::iqn_group_prep_kernel, dim3(pack_blocks + rng_blocks, G), dim3(256), 0, s, table, stale, n, cvar, pack_blocks, eps, actions_dev,
                       listed ? 1 : 0);
    const dim3 grid(group_act_grid(g), G), block(64 * sp::WAVES);
    const size_t lds = sp::LDS_ACT_FLOATS * sizeof(float);
    if (listed) hipLaunchKernelGGL(sp::iqn_group_act_kernel<true>, grid, block, lds, s, table, obs_dev, eps, actions_dev, n);
    else hipLaunchKernelGGL(sp::iqn_group_act_kernel<false>, grid, block, lds, s, table, obs_dev, eps, actions_dev, n);
    return hipGetLastError() == hipSuccess ? MN_OK : MN_ERR_HIP;
}

#include "mfma_probe.h"
