// iqn_act_few.h -- the act launch of a SHORT list of greedy rows (GreedyRows, iqn_act_common.h), without the LDS weight image.
// Included by iqn_act.hip inside its anonymous namespace, after iqn_act_split.h (uses its helpers and the layout of its weight image).
//
// Why: at eps ~ 1 the preparation launch lists a few dozen of the launch's rows.  The listed form of iqn_qvals_split_kernel then has every workgroup
// that owns a list position copy the 154-KB image into LDS, meet at a barrier, and only then start ONE wavefront on the row's chain of dependent loads
// and its 372 matrix instructions.  A wavefront that evaluates one row reads every weight operand exactly once, so the image can be read straight from
// global memory (L2): [tile][hi, lo][64 lanes] in 16-byte units is already the coalesced order.  Here
//   * a workgroup is two wavefronts and a few KB of static LDS (the feature buffers and the tau-mean hand-off);
//   * workgroup b takes list positions b, b + gridDim.x, ..., wavefront w the column tile nt = w of the row (taus 16 w .. 16 w + 15): the two tiles of a
//     row are independent through layers 1 to 3 and meet at the tau mean, where wavefront 1 parks its 16 values per lane in LDS and wavefront 0 adds them;
//   * the count, the first list entry and the first weight operands are requested at the top of the kernel, the taus / observation row as soon as the
//     entry is there, and the weights stream through a ring of FEW_DEPTH groups of four 16-byte loads per lane, refilled as they are consumed.
// Same results, bit for bit: every accumulator sees the MFMA sequence stage<> / tail issue for it (layer 1: bias, then per cos K block lo.hi, hi.lo,
// hi.hi; layers 2, 3: per K block the same three), the VALU expressions are the shared helpers or the same lines, and the tau mean adds tile 0 + tile 1
// before the row sum, as q_mean does.  A listed row is greedy: no exploration, no Q-value or quantile output, no late rows.

namespace sp {

constexpr int FEW_WAVES = 2;
constexpr int FEW_DEPTH = 8;      // weight groups in flight per wavefront (16 VGPRs each)
constexpr int FEW_PRE = 4;        // ... of which requested before the count is known (every workgroup of the grid pays for these)
constexpr int FEW_MID = 4;        // ... and before the encoders run: no more (the rest behind them; with 6, the encoders' own 26 loads no longer fit and values spill)

// The weight groups in the order a wavefront consumes them.  L1: a = feature tile (loads: kb 0 hi, lo, kb 1 hi, lo; a fifth: the tile's bias);
// L2: a = K block, b = half (output tiles 2 b, 2 b + 1: hi, lo each); L3: a = K block, b = half; B2, B3: the biases of the four output tiles; W4: the f32
// output layer's four tiles.
constexpr int FEW_L1 = 0, FEW_L2 = 1, FEW_B2 = 2, FEW_L3 = 3, FEW_B3 = 4, FEW_W4 = 5;
struct FewGrp { int kind, a, b; };
constexpr FewGrp few_group(int gi) {
    int k = 0;
    for (int t = 0; t < 4; ++t, ++k) if (k == gi) return {FEW_L1, t, 0};                    // stages -2, -1
    for (int B = 0; B < KB2 - 1; ++B) {                                                     // stage B: layer 2 block B, layer 1 block B + 2
        for (int h = 0; h < 2; ++h, ++k) if (k == gi) return {FEW_L2, B, h};
        for (int t = 2 * B + 4; t < 2 * B + 6 && t < T1; ++t, ++k) if (k == gi) return {FEW_L1, t, 0};
    }
    for (int h = 0; h < 2; ++h, ++k) if (k == gi) return {FEW_L2, KB2 - 1, h};              // the tail
    if (k++ == gi) return {FEW_B2, 0, 0};
    for (int kb = 0; kb < 2; ++kb)
        for (int h = 0; h < 2; ++h, ++k) if (k == gi) return {FEW_L3, kb, h};
    if (k++ == gi) return {FEW_B3, 0, 0};
    if (k++ == gi) return {FEW_W4, 0, 0};
    return {-1, 0, 0};
}
constexpr int few_index(int kind, int a, int b) {
    for (int gi = 0; gi < 64; ++gi) {
        const FewGrp g = few_group(gi);
        if (g.kind < 0) break;
        if (g.kind == kind && g.a == a && g.b == b) return gi;
    }
    return -1;
}
constexpr int FEW_GROUPS = few_index(FEW_W4, 0, 0) + 1;
static_assert(FEW_GROUPS == T1 + 2 * KB2 + 4 + 3, "every weight operand of a row once, and the three groups of f32 constants");
// 16-byte unit of load j of group gi, without the lane (weights, W4) or the lane group (biases)
constexpr int few_unit(int gi, int j) {
    const FewGrp g = few_group(gi);
    if (g.kind == FEW_L1) return j < 4 ? W1_U4 + (4 * g.a + j) * 64 : (OFF_B1 >> 2) + 4 * g.a;
    if (g.kind == FEW_L2) return W2_U4 + (((2 * g.b + (j >> 1)) * KB2 + g.a) * 2 + (j & 1)) * 64;
    if (g.kind == FEW_L3) return W3_U4 + (((2 * g.b + (j >> 1)) * 2 + g.a) * 2 + (j & 1)) * 64;
    if (g.kind == FEW_B2) return (OFF_B2 >> 2) + 4 * j;
    if (g.kind == FEW_B3) return (OFF_B3 >> 2) + 4 * j;
    return (OFF_W4 >> 2) + j * 64;
}
static_assert(OFF_B1 % 4 == 0 && OFF_B2 % 4 == 0 && OFF_B3 % 4 == 0 && OFF_W4 % 4 == 0, "16-byte aligned blocks");

typedef u32x4 FewRing[FEW_DEPTH][5];

// requests group GI into its ring slot (GI % FEW_DEPTH); nothing behind the last group
// (addresses: a uniform pointer to the unit + the lane's 32-bit byte offset, so that a load is one instruction on a scalar base and ONE offset register;
// written as p4[unit + lane] every load gets a 64-bit address pair of its own, computed in front of the position loop and spilled)
typedef const __attribute__((address_space(1))) char *FewImage;      // (global, said explicitly: the pointer passes through an asm per position, see the kernel)
struct FewOff { uint32_t lane, group; FewImage image; };      // 16 lane, 16 (lane >> 4), the image
__device__ __forceinline__ u32x4 few_ld(const FewOff &o, int unit, uint32_t off) {
    return *reinterpret_cast<const __attribute__((address_space(1))) u32x4 *>(o.image + 16 * unit + off);
}
template <int GI>
__device__ __forceinline__ void few_load(FewRing &ring, const FewOff &o) {
    if constexpr (GI < FEW_GROUPS) {
        constexpr FewGrp G = few_group(GI);
        constexpr int s = GI % FEW_DEPTH;
        constexpr bool by_group = G.kind == FEW_B2 || G.kind == FEW_B3;
        static_for<4>([&](auto J_) {
            constexpr int j = decltype(J_)::value;
            ring[s][j] = few_ld(o, few_unit(GI, j), by_group ? o.group : o.lane);
        });
        if constexpr (G.kind == FEW_L1) ring[s][4] = few_ld(o, few_unit(GI, 4), o.group);
    }
}

// Stage B of the fused layers 1 + 2 for ONE column tile, as stage<B> (iqn_act_split.h) runs it for two: the 12 layer-2 MFMAs of K block B, the layer-1
// MFMAs of block B + 2 (into accW) and the epilogue of block B + 1 (accR -> bhN / blN), the two kinds of MFMA alternating so that no accumulator's
// chain waits for itself.  A group's slot is refilled behind the last MFMA that reads it.
template <int B>
__device__ __forceinline__ void few_stage(FewRing &ring, const FewOff &o, const f32x4 *__restrict__ fbv,
                                          const f16x8 (&cbh)[2], const f16x8 (&cbl)[2], const f16x8 bh, const f16x8 bl, f32x4 (&acc2)[4],
                                          f32x4 (&accW)[2], const f32x4 (&accR)[2], f16x8 &bhN, f16x8 &blN) {
    constexpr int NTI_W = (B + 2 < KB2) ? ntiles_of(B + 2) : 0;
    constexpr int NTI_R = (B + 1 >= 0 && B + 1 < KB2) ? ntiles_of(B + 1) : 0;
    constexpr int N_L2 = B >= 0 ? 12 : 0, N_L1 = 6 * NTI_W, N_MIX = 2 * (N_L2 < N_L1 ? N_L2 : N_L1), NM = N_L2 + N_L1;
    constexpr int N_UNIT = NTI_R * 2;
    f32x4 fv[2];
#pragma unroll
    for (int ti = 0; ti < NTI_R; ++ti) fv[ti] = fbv[4 * (2 * (B + 1) + ti)];          // S 2^-k1 features[16t + 4g + r]
    const f16x2 zero2 = {(_Float16)0.f, (_Float16)0.f};
    f16x2 hP[4] = {zero2, zero2, zero2, zero2}, lP[4] = {zero2, zero2, zero2, zero2};
    __builtin_amdgcn_sched_barrier(0);
    static_for<NM>([&](auto M_) {
        constexpr int m = decltype(M_)::value;
        constexpr bool is_l2 = m < N_MIX ? (m % 2 == 0) : (N_L2 > N_L1);
        constexpr int idx = m < N_MIX ? m / 2 : m - N_MIX / 2;
        if constexpr (is_l2) {
            constexpr int p = idx / 4, mt = idx % 4;
            constexpr int gi = few_index(FEW_L2, B, mt / 2), s = gi % FEW_DEPTH;
            const f16x8 ah = __builtin_bit_cast(f16x8, ring[s][2 * (mt & 1)]), al = __builtin_bit_cast(f16x8, ring[s][2 * (mt & 1) + 1]);
            acc2[mt] = mf(p == 0 ? al : ah, p == 1 ? bl : bh, acc2[mt]);
            if constexpr (p == 2 && (mt & 1)) few_load<gi + FEW_DEPTH>(ring, o);
        } else {
            constexpr int kb = idx / (3 * NTI_W), p = (idx % (3 * NTI_W)) / NTI_W, ti = idx % NTI_W;
            constexpr int gi = few_index(FEW_L1, 2 * (B + 2) + ti, 0), s = gi % FEW_DEPTH;
            const f16x8 ah = __builtin_bit_cast(f16x8, ring[s][2 * kb]), al = __builtin_bit_cast(f16x8, ring[s][2 * kb + 1]);
            accW[ti] = mf(p == 0 ? al : ah, p == 1 ? cbl[kb] : cbh[kb], (kb == 0 && p == 0) ? __builtin_bit_cast(f32x4, ring[s][4]) : accW[ti]);
            if constexpr (kb == 1 && p == 2) few_load<gi + FEW_DEPTH>(ring, o);
        }
        // ---- the epilogue of one register pair (ReLU, Hadamard, split) behind MFMA (u + 1) NM / (N_UNIT + 1)
#pragma unroll
        for (int u = 0; u < N_UNIT; ++u) {
            if ((u + 1) * NM / (N_UNIT + 1) == m) {
                const int ti = u / 2, pr = u % 2;
                float x0 = relu1(accR[ti][2 * pr]), x1 = relu1(accR[ti][2 * pr + 1]);
                x0 *= fv[ti][2 * pr]; x1 *= fv[ti][2 * pr + 1];
                const f16x2 hcur = cvt_pair(x0, x1);
                const float r0 = residual_lo32(x0, hcur), r1 = residual_hi32(x1, hcur);
                hP[2 * ti + pr] = hcur;
                lP[2 * ti + pr] = cvt_pair(r0, r1);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    });
    if (N_UNIT > 0) {
        bhN = cat4(hP[0], hP[1], hP[2], hP[3]);
        blN = cat4(lP[0], lP[1], lP[2], lP[3]);
    }
}

// The end of the row's pipeline for one column tile, as tail (iqn_act_split.h): layer 2's last K block (output tiles 0, 1, then 2, 3), the layer-2
// epilogue (unscale + bias, ReLU, split) of a half under the MFMAs that follow it, layer 3's two K blocks.  c2 = 2^-k2 S2 / S1, S = S2.
__device__ __forceinline__ void few_tail(FewRing &ring, const FewOff &o, float c2, float S, const f16x8 bh, const f16x8 bl,
                                         f32x4 (&acc2)[4], f32x4 (&acc3)[4]) {
    constexpr int sB2 = few_index(FEW_B2, 0, 0) % FEW_DEPTH;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc3[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 sb[4];
    f16x2 hP[2][4], lP[2][4];
    f16x8 b3h[2], b3l[2];
    __builtin_amdgcn_sched_barrier(0);
    static_for<36>([&](auto M_) {
        constexpr int m = decltype(M_)::value;
        if constexpr (m < 12) {                 // layer 2, last K block: tiles {0, 1} then {2, 3}
            constexpr int half = m / 6, q = m % 6, p = q / 2, mt = 2 * half + q % 2;
            constexpr int gi = few_index(FEW_L2, KB2 - 1, half), s = gi % FEW_DEPTH;
            const f16x8 ah = __builtin_bit_cast(f16x8, ring[s][2 * (mt & 1)]), al = __builtin_bit_cast(f16x8, ring[s][2 * (mt & 1) + 1]);
            acc2[mt] = mf(p == 0 ? al : ah, p == 1 ? bl : bh, acc2[mt]);
            if constexpr (p == 2 && (mt & 1)) few_load<gi + FEW_DEPTH>(ring, o);
        } else {                                // layer 3, K block 0 then 1
            constexpr int kb = (m - 12) / 12, q = (m - 12) % 12, p = q / 4, mt = q % 4;
            constexpr int gi = few_index(FEW_L3, kb, mt / 2), s = gi % FEW_DEPTH;
            const f16x8 ah = __builtin_bit_cast(f16x8, ring[s][2 * (mt & 1)]), al = __builtin_bit_cast(f16x8, ring[s][2 * (mt & 1) + 1]);
            acc3[mt] = mf(p == 0 ? al : ah, p == 1 ? b3l[kb] : b3h[kb], acc3[mt]);
            if constexpr (p == 2 && (mt & 1)) few_load<gi + FEW_DEPTH>(ring, o);
        }
        if constexpr (m == 5) {                 // the biases, S b2 (their group is behind layer 2's last one)
#pragma unroll
            for (int t = 0; t < 4; ++t) sb[t] = __builtin_bit_cast(f32x4, ring[sB2][t]) * S;
            few_load<few_index(FEW_B2, 0, 0) + FEW_DEPTH>(ring, o);
        }
        // epilogue units (2 halves x 2 tiles x 2 register pairs): half 0 behind slots 6..9, half 1 behind slots 12..15
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if ((u < 4 ? 6 + u : 8 + u) == m) {
                const int half = u / 4, ti = (u % 4) / 2, pr = u % 2, t = 2 * half + ti;
                const float t0 = relu1(fmaf(acc2[t][2 * pr], c2, sb[t][2 * pr])), t1 = relu1(fmaf(acc2[t][2 * pr + 1], c2, sb[t][2 * pr + 1]));
                const f16x2 hcur = cvt_pair(t0, t1);
                float r0, r1;
                residual_pair(t0, t1, hcur, r0, r1);
                hP[half][2 * ti + pr] = hcur;
                lP[half][2 * ti + pr] = cvt_pair(r0, r1);
                if (u % 4 == 3) {
                    b3h[half] = cat4(hP[half][0], hP[half][1], hP[half][2], hP[half][3]);
                    b3l[half] = cat4(lP[half][0], lP[half][1], lP[half][2], lP[half][3]);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    });
}

__global__ __launch_bounds__(64 * FEW_WAVES, 2) void iqn_act_few_kernel(const float *__restrict__ obs, const float *__restrict__ taus,
                                                                        const uint32_t *__restrict__ packed, int32_t *__restrict__ actions, int n,
                                                                        uint64_t *__restrict__ rng_state, const GreedyRows rows) {
    __shared__ __attribute__((aligned(16))) float s_fb[FEW_WAVES * F];      // per-wave scaled features
    __shared__ __attribute__((aligned(16))) float s_h3[16 * 64];            // wavefront 1's layer-3 activations, [value][lane]
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, g = lane >> 4;
    const int col = lane & 15;
    const float *pf = reinterpret_cast<const float *>(packed);
    const f32x4 *pv = reinterpret_cast<const f32x4 *>(packed);
    // ---- everything that does not depend on the row is requested first: the count words and the first list entry (in bounds whatever the count is;
    // used only if the position is inside the list), the first weight groups, the constants
    const uint32_t wd[3] = {rows.words[0], rows.words[1], rows.words[2]};      // (not words[3]: a loaded word nobody reads is a register the next instructions wait for)
    const int pos0 = blockIdx.x;
    const int row0 = rows.list[pos0 < n ? pos0 : n - 1];
    __builtin_amdgcn_sched_barrier(0);
    const char *image = reinterpret_cast<const char *>(packed);
    FewOff o = {16u * (uint32_t)lane, 16u * (uint32_t)g, (FewImage)image};
    asm volatile("" : "+v"(o.lane), "+v"(o.group));
    FewRing ring;
    static_for<FEW_PRE>([&](auto I_) { few_load<decltype(I_)::value>(ring, o); });
    const float c1 = pf[OFF_CST + 0], c2 = pf[OFF_CST + 1], c3 = pf[OFF_CST + 2];
    const float a2 = pf[OFF_CST + 3], d2 = pf[OFF_CST + 4], a3 = pf[OFF_CST + 5], d3 = pf[OFF_CST + 6];
    const float b4c = pf[OFF_B4 + col];
    const uint32_t slot = wd[2] & 1u, count = slot ? wd[1] : wd[0];
    const int n_rows = count < (uint32_t)n ? (int)count : n;
    if (pos0 == 0 && tid == 0) {
        if (rng_state) rng_state[1] += 1;       // the draws of this call were made by the preparation launch
        rows.words[3] = slot ^ 1u;              // the next call counts in the other slot
    }
    if (pos0 >= n_rows) return;

    const int fb_f = wave * F + lane;           // this wave's feature buffer (floats)
    const f32x4 *fbv = reinterpret_cast<const f32x4 *>(s_fb) + ((wave * F) >> 2) + g;
    const float hk0 = 4.0f * (float)g;          // cos(tau pi k), k = 32 kb + 8 g + i, in revolutions: k / 2 = hk0 + (16 kb + i / 2)
    // one listed row (its first weight groups requested by the caller); the same for both wavefronts of the workgroup, which meet at its barrier
    const auto eval_row = [&](int row) __attribute__((always_inline)) {
        row = __builtin_amdgcn_readfirstlane(row);
        // (made opaque per position: as invariants of the loop the addresses built on them are all computed in front of it)
        int enc_w = (OFF_WS >> 2) + lane;       // sensor encoder weights (16-byte units)
        int enc_f = OFF_BND + lane;             // bounds / encoder biases (floats)
        float hk = hk0;
        asm volatile("" : "+v"(o.lane), "+v"(o.group), "+v"(enc_w), "+v"(enc_f), "+v"(hk), "+s"(image));
        o.image = (FewImage)image;
        if ((unsigned)row < (unsigned)n) {
            const float tau = taus[(size_t)row * K_TAUS + 16 * wave + col];
            const float *orow = obs + (size_t)row * OBS;
            float ov[28];
#pragma unroll
            for (int i = 0; i < 28; ++i) ov[i] = i < OBS ? orow[i] : 0.f;
            static_for<FEW_MID - FEW_PRE>([&](auto I_) { few_load<FEW_PRE + decltype(I_)::value>(ring, o); });
            // layer-1 B operands: the cos embedding (model.py:155), unscaled, split
            f16x8 cbh[2], cbl[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                f16x2 h[4], l[4];
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    split2(__builtin_amdgcn_cosf(tau * (hk + (16.0f * kb + 0.5f * (2 * p)))),
                           __builtin_amdgcn_cosf(tau * (hk + (16.0f * kb + 0.5f * (2 * p + 1)))), h[p], l[p]);
                cbh[kb] = cat4(h[0], h[1], h[2], h[3]);
                cbl[kb] = cat4(l[0], l[1], l[2], l[3]);
            }
            // observation encoders (their weights read from the image in global memory), per-row scales, S 2^-k1 features -> this wave's LDS buffer
            EncState st;
            static_for<N_ENC_SUB>([&](auto I_) { enc_substep<decltype(I_)::value>(pf, pv, enc_w, enc_f, lane, ov, st); });
            const EnvScale sc = env_scale(st.bnd, a2, d2, a3, d3);
            store_features(s_fb, fb_f, lane, st, sc.S1 * c1);
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            static_for<FEW_DEPTH - FEW_MID>([&](auto I_) { few_load<FEW_MID + decltype(I_)::value>(ring, o); });

            f32x4 acc2[4], acc3[4], accA[2], accB[2];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc2[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            f16x8 bhA, blA, bhB, blB;
            bhA = blA = bhB = blB = __builtin_bit_cast(f16x8, (u32x4){0u, 0u, 0u, 0u});
            few_stage<-2>(ring, o, fbv, cbh, cbl, bhB, blB, acc2, accA, accB, bhB, blB);      // layer-1 block 0
            few_stage<-1>(ring, o, fbv, cbh, cbl, bhB, blB, acc2, accB, accA, bhA, blA);      // layer-1 block 1, epilogue of block 0
            few_stage<0>(ring, o, fbv, cbh, cbl, bhA, blA, acc2, accA, accB, bhB, blB);
            few_stage<1>(ring, o, fbv, cbh, cbl, bhB, blB, acc2, accB, accA, bhA, blA);
            few_stage<2>(ring, o, fbv, cbh, cbl, bhA, blA, acc2, accA, accB, bhB, blB);
            few_stage<3>(ring, o, fbv, cbh, cbl, bhB, blB, acc2, accB, accA, bhA, blA);
            few_stage<4>(ring, o, fbv, cbh, cbl, bhA, blA, acc2, accA, accB, bhB, blB);
            few_stage<5>(ring, o, fbv, cbh, cbl, bhB, blB, acc2, accB, accA, bhA, blA);
            few_tail(ring, o, c2 * sc.r21, sc.S2, bhA, blA, acc2, acc3);

            // ---- layer 3 epilogue of this tile; the tau mean over both tiles, the f32 output layer and the argmax in wavefront 0 (as q_mean)
            constexpr int sB3 = few_index(FEW_B3, 0, 0) % FEW_DEPTH, sW4 = few_index(FEW_W4, 0, 0) % FEW_DEPTH;
            const float c3e = c3 * sc.r32;      // layer-3 accumulators carry S2 2^k3: to S3
            f32x4 hv[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const f32x4 sb = __builtin_bit_cast(f32x4, ring[sB3][mt]) * sc.S3;
                hv[mt] = relu4s(fma4(acc3[mt], c3e, sb));
            }
            if (wave == 1) {
#pragma unroll
                for (int i = 0; i < 16; ++i) s_h3[i * 64 + lane] = hv[i >> 2][i & 3];
            }
            __syncthreads();
            if (wave == 0) {
                float hs[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) hs[i] = hv[i >> 2][i & 3] + s_h3[i * 64 + lane];      // tile 0 + tile 1, then the row sum
                row_sum16_x16(hs);
                float part = 0.f;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const f32x4 a = __builtin_bit_cast(f32x4, ring[sW4][mt]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) part = fmaf(a[r], hs[4 * mt + r], part);
                }
                part = sum_rows4(part);
                const float qv = part * (sc.invS3 * (1.0f / K_TAUS)) + b4c;      // Q(s, action = col), valid for col < 9
                float best = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qv), 0));
                int arg = 0;
#define SP_ARG(a) { const float v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qv), a)); if (v > best) { best = v; arg = a; } }
                SP_ARG(1) SP_ARG(2) SP_ARG(3) SP_ARG(4) SP_ARG(5) SP_ARG(6) SP_ARG(7) SP_ARG(8)
#undef SP_ARG
                if (lane == 0) actions[row] = arg;
            }
        }
    };
    // the first position as straight-line code (what a short list runs: nothing of it waits at a loop header), any further ones in a loop
    eval_row(row0);
    for (int pos = pos0 + (int)gridDim.x; pos < n_rows; pos += (int)gridDim.x) {
        __syncthreads();      // wavefront 0 has read the hand-off of the row before
        const int row = rows.list[pos];
        static_for<FEW_PRE>([&](auto I_) { few_load<decltype(I_)::value>(ring, o); });
        eval_row(row);
    }
}

}  // namespace sp
