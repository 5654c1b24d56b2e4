// mn_prep_reset.hip -- the episode resets of vector step t and the preparation of act call t + 1 in ONE launch on the caller's stream (gfx950).
//
// With a short act launch (eps near 1: only the rows that do not explore go through the network) the chain from one step kernel to the next is
//     step(t) -> event -> reset(t) on the handle's side stream -> event -> step(t + 1)
// and the draw and act launches of t + 1 finish beside the reset: nothing hides the reset's single-wavefront latency chain or the two cross-stream events.
// The draws of an act call need the generator counter, eps and the weights, not the observations, so they share a launch with the resets:
//     step(t) -> [ resets(t) | pack blocks of a stale weight image | draws(t + 1) ] -> act(t + 1), no late rows -> step(t + 1)
// No side stream, no events, no `ready` words; the blocks of the launch are independent of each other and everything behind it is ordered by the stream.
//
//   blocks [0, R)                    one reset wavefront each, queue-driven exactly as mn_reset_kernel with the sharded done-queue (MnDoneQueue, mn_note_count,
//                                    mn_reset_env<M, PARITY, MtDoubles> in its short-chain form, ready = NULL); first in the grid, so the long chains start first.
//                                    The array pointers its stores need come from the handle's device copy of MnArrays (A_mem: mn_reset_env's TAIL_MEM)
//   blocks [R, R + pack)             the weight image when it is stale: one 32-bit word per thread (sp::pack_word, as iqn_split_prep_kernel)
//   blocks [R + pack, gridDim.x)     draw_block<ROWS, 64>: the call's taus and exploration uniforms, with `rows` the exploring rows' actions and the list of the others
// The workgroup is ONE wavefront (the reset body's __syncthreads() are wave barriers), so the pack and draw blocks are 64 threads wide; the draws are
// counter-based and do not depend on the block shape.  Those blocks inherit the reset body's register and LDS allocation (3 136 B; ~125 registers in both
// precisions: a SIMD holds four of them), which costs an otherwise empty chip nothing; no scratch (tests/test_reset_in_prep_cpu.py, tests/test_reset_chain_cpu.py).
//
// Both roundings in one file, as mn_rollout_iqn.o: built with -ffp-contract=fast-honor-pragmas; the reset body under `#pragma clang fp contract(off)` is
// mn_reset.o's code (world generation stays bit-identical to numpy), the pack and the draws are iqn_act.o's (contraction allowed).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "marinenav_hip.h"

#pragma clang fp contract(off)
#include "mn_reset_body.h"
#include "mn_done_queue.h"
#pragma clang fp contract(fast)

namespace {

#include "iqn_act_common.h"
#include "iqn_act_split.h"

constexpr int PR_PACK_BLOCKS = (sp::OFF_FB + MN_WAVE - 1) / MN_WAVE;

struct PrepArgs {      // what sp::iqn_split_prep_kernel takes
    IqnWeights w;
    const float *consts;
    uint32_t *packed;
    const uint64_t *rng_state;
    float *draws;
    int n;
    const float *cvar_row;
    float cvar;
    int pack_blocks;      // PR_PACK_BLOCKS when the image is stale, else 0
    float eps;
    int32_t *actions;
    GreedyRows rows;
};

template <typename M, bool PARITY>
__global__ __launch_bounds__(MN_WAVE) void mn_prep_reset_kernel(MnArrays A, MnDev P, const uint32_t *__restrict__ count_dev, const int32_t *__restrict__ list,
                                                                float *__restrict__ obs_out, const MnSeen seen, int reset_blocks, const MnArrays *A_mem, PrepArgs a) {
    __shared__ MtDblLds S;
    __shared__ WorldLds W;
    if ((int)blockIdx.x < reset_blocks) {
        MnDoneQueue Q;
        const uint32_t count = Q.open(count_dev);
        mn_note_count(seen, count);      // (block 0 is a reset block: reset_blocks >= 1)
        for (uint32_t qi = blockIdx.x; qi < count; qi += (uint32_t)reset_blocks) mn_reset_env<M, PARITY, MtDoubles, true, true>(A, P, S, W, Q.at(list, A.qcap, qi), 0, obs_out, nullptr, 0u, A_mem);
        return;
    }
    const int b = (int)blockIdx.x - reset_blocks;
    if (b < a.pack_blocks) {
        const int i = b * MN_WAVE + (int)threadIdx.x;
        if (i < sp::OFF_FB) a.packed[i] = sp::pack_word(a.w, a.consts, i);
        return;
    }
    if (a.rows.words) draw_block<true, MN_WAVE>(a.rng_state, a.draws, a.n, a.cvar_row, a.cvar, reset_blocks + a.pack_blocks, a.eps, a.actions, a.rows);
    else draw_block<false, MN_WAVE>(a.rng_state, a.draws, a.n, a.cvar_row, a.cvar, reset_blocks + a.pack_blocks);
}

}  // namespace

// Reset wavefronts of a launch from the decaying peak of the episodes a launch starts (`seen`, as the host reads it; 0xffffffff: none seen yet): a few times
// the peak, so that a step with more episode ends than the last ones still gets a wavefront per entry, with a floor, and capped like mn_launch_reset's
// grid.  Every wavefront loops over the queue entries, so any count is correct.
int mn_prep_reset_blocks(uint32_t seen, int n) {
    long r = seen == 0xffffffffu ? MN_PREP_RESET_MAX_BLOCKS : 4L * (long)seen;
    if (r < MN_PREP_RESET_MIN_BLOCKS) r = MN_PREP_RESET_MIN_BLOCKS;
    if (r > MN_PREP_RESET_MAX_BLOCKS) r = MN_PREP_RESET_MAX_BLOCKS;
    if (r > n) r = n;
    return r < 1 ? 1 : (int)r;
}

void mn_launch_prep_reset(const MnOwedReset &o, const MnPrepLaunch &p, hipStream_t s) {
    const MnSeen seen = {o.peak_dev, o.peak_host};
    PrepArgs a;
    const float *const *w = p.weights;
    a.w = {w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12], w[13]};
    a.consts = p.consts; a.packed = p.packed; a.rng_state = p.rng_state; a.draws = p.draws; a.n = p.n; a.cvar_row = p.cvar_row; a.cvar = p.cvar;
    a.pack_blocks = p.pack ? PR_PACK_BLOCKS : 0;
    a.eps = p.eps; a.actions = p.actions; a.rows = GreedyRows{p.rows_list, p.rows_words};
    const long items = ((long)p.n * (K_TAUS + 1) + 3) / 4;
    long draw = (items + MN_WAVE - 1) / MN_WAVE;
    if (draw > p.max_draw_blocks) draw = p.max_draw_blocks;
    if (draw < 1) draw = 1;
    const dim3 grid((unsigned)(o.blocks + a.pack_blocks + draw));
    if (o.ev_begin) (void)hipEventRecord(o.ev_begin, s);
    if (o.precision == MN_PRECISION_F64)
        hipLaunchKernelGGL((mn_prep_reset_kernel<double, true>), grid, dim3(MN_WAVE), 0, s, *o.A, *o.P, o.count_dev, o.list, o.obs, seen, o.blocks, o.A_mem, a);
    else
        hipLaunchKernelGGL((mn_prep_reset_kernel<float, false>), grid, dim3(MN_WAVE), 0, s, *o.A, *o.P, o.count_dev, o.list, o.obs, seen, o.blocks, o.A_mem, a);
    if (o.ev_end) (void)hipEventRecord(o.ev_end, s);
}
