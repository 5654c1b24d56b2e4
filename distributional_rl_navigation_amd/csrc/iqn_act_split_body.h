// iqn_act_split_body.h -- the body of sp::iqn_qvals_split_kernel (iqn_act_split.h), included as text by that kernel and by the grouped act kernels of
// iqn_act_group.h: ONE source and one arithmetic sequence per output element, whatever kernel it is compiled into.  The including kernel provides, as
// parameters or locals of these names: obs, taus, packed, qvals, explore_u, eps, actions, n, rng_state, quantiles, h1, late (LateRows), rows (GreedyRows),
// and the compile-time QUANT, SHARED, NW, LATE, ROWS.  blockIdx.x / gridDim.x are the workgroup's index and the workgroup count among those that share
// these arguments: a grouped launch keeps its group in blockIdx.y.
    static_assert(!LATE || (!QUANT && !SHARED), "late rows: the acting form with per-environment taus");
    static_assert(!ROWS || (!QUANT && !SHARED), "listed rows: the acting form with per-environment taus");
#ifndef SP_LATE_PRIO
#define SP_LATE_PRIO 0
#endif
    if constexpr (LATE) __builtin_amdgcn_s_setprio(SP_LATE_PRIO);      // the reset wavefronts that share these SIMDs take the issue slots this kernel leaves
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    if (rng_state && blockIdx.x == 0 && tid == 0) rng_state[1] += 1;   // the draws of this call were made by the prep kernel
    [[maybe_unused]] int n_rows = 0;       // ROWS: length of the list
    if constexpr (ROWS) {
        const uint32_t slot = rows.words[2] & 1u, count = rows.words[slot];
        n_rows = count < (uint32_t)n ? (int)count : n;
        if (blockIdx.x == 0 && tid == 0) rows.words[3] = slot ^ 1u;      // the next call counts in the other slot
        if ((int)blockIdx.x >= n_rows) return;
    }
    // the acting form has no use for the output layer's MFMA operands (act_eval's quantiles): its feature buffers sit there, and the 4 KB
    // that frees are what lets a reset workgroup (3.1 KB of LDS) share the CU with this one
    constexpr int IMG = QUANT ? OFF_FB : OFF_W4H;
    {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(packed);
        u32x4 *dst = reinterpret_cast<u32x4 *>(lds);
        if constexpr (SHARED) {      // the layer-1 constant takes the place of the layer-1 weights
            const u32x4 *hsrc = reinterpret_cast<const u32x4 *>(h1);
            for (int i = tid; i < H1_FLOATS / 4; i += blockDim.x) dst[i] = hsrc[i];
            for (int i = W2_U4 + tid; i < IMG / 4; i += blockDim.x) dst[i] = src[i];
        } else {
            for (int i = tid; i < IMG / 4; i += blockDim.x) dst[i] = src[i];
        }
    }
    __syncthreads();

    const int lane = tid & 63, g = lane >> 4, col = lane & 15;
    const int wave = tid >> 6, waves_per_block = blockDim.x >> 6;
    const f32x4 *ldsv = reinterpret_cast<const f32x4 *>(lds);
    const u32x4 *lds4 = reinterpret_cast<const u32x4 *>(lds);
    LdsBase lb;
    // per-wave feature buffer: behind the image; shared-tau form: in the rest of the W1 region, behind the layer-1 constant
    constexpr int FB0 = SHARED ? H1_FLOATS : IMG;
    static_assert(!SHARED || H1_FLOATS + NW * F <= W2_U4 * 4, "feature buffers of the shared-tau kernel fit into the W1 region");
    static_assert(SHARED || NW <= WAVES, "feature buffers behind the image: WAVES of them");
    lb.w_lo = lane; lb.w_hi = lane + 4096; lb.fl = (OFF_B1 >> 2) + g; lb.fb = ((FB0 + wave * F) >> 2) + g;
    int enc_w = (OFF_WS >> 2) + lane;       // sensor encoder weights (16-byte units)
    int enc_f = OFF_BND + lane;             // bounds / encoder biases (floats)
    int fb_f = FB0 + wave * F + lane;       // this wave's feature buffer (floats)
    asm volatile("" : "+v"(lb.w_lo), "+v"(lb.w_hi), "+v"(lb.fl), "+v"(lb.fb), "+v"(enc_w), "+v"(enc_f), "+v"(fb_f));
    const float c1 = lds[OFF_CST + 0], c2 = lds[OFF_CST + 1], c3 = lds[OFF_CST + 2];
    const float a2 = lds[OFF_CST + 3], d2 = lds[OFF_CST + 4], a3 = lds[OFF_CST + 5], d3 = lds[OFF_CST + 6];

    // cos(tau * pi * k), k = 32 kb + 8 g + i: v_cos_f32 takes its argument in revolutions (tau * k / 2 <= 32) and reduces it itself
    const float hk0 = 4.0f * (float)g;     // k / 2 = hk0 + (16 kb + i / 2)

    // Software-pipelining the loop ACROSS environments (next environment's taus / observation row loaded and its encoders run in
    // the pipeline's issue gaps) was built and measured: 359 us against 326 us -- the kernel is
    // bound by the SIMD's aggregate instruction issue (~1 instruction per 5 cycles over both waves, the same rate as
    // profiles/r02_mfma_valu_overlap_probe.txt at K = 3), so moving instructions around buys nothing and the extra live
    // registers cost spills.  Requesting ONLY the next environment's taus and observation row one iteration ahead (2 VGPRs,
    // 28 SGPRs) changes nothing either (338 vs 337 us, alternating runs on one GPU): that latency is covered by the partner wave.
    [[maybe_unused]] int sp_iter = 0;
    // layer-1 B operands: the cos embedding (model.py:155), unscaled, split.  Computed here for a wave's FIRST environment only; for every
    // later one by the CosJob pieces inside stage 5 / the tail of the environment before it (same expressions, same bits).
    f16x8 cbh[2][NT], cbl[2][NT];
    CosJob cj;
    cj.hk0 = hk0;
    // the wave's rows: e_first + k e_stride; ROWS: the rows at those positions of the list
    const int e_first = ROWS ? blockIdx.x + gridDim.x * wave : blockIdx.x * waves_per_block + wave, e_stride = gridDim.x * waves_per_block;
    [[maybe_unused]] const auto listed = [&](int pos) {      // (wave-uniform) row at list position `pos`, n behind the list's end
        pos = __builtin_amdgcn_readfirstlane(pos);
        const int r = pos < n_rows ? rows.list[pos] : n;
        return (unsigned)r < (unsigned)n ? r : n;
    };
    // LATE: the wave's rows as two bit sets (bit k = row e_first + k e_stride): final observations first, late ones last
    [[maybe_unused]] unsigned long long rows_now = 0, rows_late = 0;
    [[maybe_unused]] bool is_late = false;
    [[maybe_unused]] int e_lane = 0;       // LATE && ROWS: lane k holds the row of bit k
    [[maybe_unused]] const auto row_of = [&](int k) { return ROWS ? __builtin_amdgcn_readlane(e_lane, k) : e_first + k * e_stride; };
    int e0 = e_first;
    if constexpr (LATE) {
        int e_l = e_first + lane * e_stride;
        if constexpr (ROWS) {
            const int r = e_l < n_rows ? rows.list[e_l] : n;
            e_l = e_lane = (unsigned)r < (unsigned)n ? r : n;
        }
        const bool v = e_l < n, l = v && late.mask[v ? e_l : 0] != 0;
        const unsigned long long mv = __ballot(v), ml = __ballot(l);
        rows_now = mv & ~ml; rows_late = ml;
        if (rows_now) { const int k = __builtin_ctzll(rows_now); rows_now &= rows_now - 1; e0 = row_of(k); }
        else if (rows_late) { const int k = __builtin_ctzll(rows_late); rows_late &= rows_late - 1; e0 = row_of(k); is_late = true; }
        else e0 = n;
        e0 = __builtin_amdgcn_readfirstlane(e0);
    } else if constexpr (ROWS) e0 = listed(e_first);
    if (!SHARED && e0 < n) {
        float tau[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) tau[nt] = taus[(size_t)e0 * K_TAUS + 16 * nt + col];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                f16x2 h[4], l[4];
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (SP_ABL & 8) { h[p] = __builtin_bit_cast(f16x2, tau[nt]); l[p] = h[p]; }
                    else
                    split2(__builtin_amdgcn_cosf(tau[nt] * (hk0 + (16.0f * kb + 0.5f * (2 * p)))),
                           __builtin_amdgcn_cosf(tau[nt] * (hk0 + (16.0f * kb + 0.5f * (2 * p + 1)))), h[p], l[p]);
                cbh[kb][nt] = cat4(h[0], h[1], h[2], h[3]);
                cbl[kb][nt] = cat4(l[0], l[1], l[2], l[3]);
            }
    }
    int e_follow = n;      // LATE, ROWS: the row after `e` (n: none)
    [[maybe_unused]] bool follow_late = false;
    [[maybe_unused]] int pos_ahead = e_first + e_stride, e_ahead = n;      // ROWS without LATE: list position of e_follow, and the row behind e_follow
    if constexpr (ROWS && !LATE) e_follow = listed(pos_ahead);
    for (int e = e0; e < n;) {
        [[maybe_unused]] unsigned long long tk[16];
#define SP_TICK(i) do { if (SP_ABL & 64) { __builtin_amdgcn_sched_barrier(0); tk[i] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } } while (0)
        SP_TICK(0);
        const float u_explore = (!ROWS && explore_u && eps > 0.f) ? explore_u[__builtin_amdgcn_readfirstlane(e)] : 2.0f;     // used ~10 us later
        [[maybe_unused]] const bool late_row = is_late;
        if constexpr (LATE) {
            e_follow = n; follow_late = false;
            if (rows_now) { const int k = __builtin_ctzll(rows_now); rows_now &= rows_now - 1; e_follow = row_of(k); }
            else if (rows_late) { const int k = __builtin_ctzll(rows_late); rows_late &= rows_late - 1; e_follow = row_of(k); follow_late = true; }
            e_follow = __builtin_amdgcn_readfirstlane(e_follow);
            is_late = follow_late;
        } else if constexpr (ROWS) {      // requested an iteration ahead of the taus it addresses
            pos_ahead += e_stride;
            e_ahead = listed(pos_ahead);
        }
        if constexpr (!SHARED) {   // the next environment's taus (the last iteration re-reads its own: straight-line code); consumed from stage 5 on
            const int e_nx = (LATE || ROWS) ? (e_follow < n ? e_follow : e) : (e + e_stride < n ? e + e_stride : e);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) cj.tau[nt] = taus[(size_t)e_nx * K_TAUS + 16 * nt + col];
        }
        SP_TICK(1);
        // observation encoders, per-environment scale S, S 2^-k1 features -> this wave's LDS buffer
        EnvScale sc;
        {
            const float *orow = obs + (size_t)__builtin_amdgcn_readfirstlane(e) * OBS;
            float ov[28];
            if (LATE && late_row) {      // (wave-uniform) wait for the reset wave's "row is final" word, then read the row past the caches
                const uint32_t *fp = late.flag + __builtin_amdgcn_readfirstlane(e);
                const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
                while (__hip_atomic_load(fp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != late.tick) {
                    __builtin_amdgcn_s_sleep(16);
                    if (__builtin_amdgcn_s_memrealtime() - t0 > late.bound_ticks) {
                        if (lane == 0) __hip_atomic_store(late.status_host, atomicAdd(late.status, 1u) + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        break;
                    }
                }
                const uint32_t x = __hip_atomic_load(reinterpret_cast<const uint32_t *>(orow) + (lane < OBS ? lane : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int i = 0; i < 28; ++i) ov[i] = i < OBS ? __builtin_bit_cast(float, __builtin_amdgcn_readlane((int)x, i)) : 0.f;
            } else {
#pragma unroll
            for (int i = 0; i < 28; ++i) ov[i] = i < OBS ? orow[i] : 0.f;
            }
            EncState st;
            static_for<N_ENC_SUB>([&](auto I_) { enc_substep<decltype(I_)::value>(lds, ldsv, enc_w, enc_f, lane, ov, st); });
            sc = env_scale(st.bnd, a2, d2, a3, d3);
            store_features(lds, fb_f, lane, st, SHARED ? sc.S1 : sc.S1 * c1);      // (the shared layer-1 constant carries no 2^k1)
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }

        SP_TICK(2);
        // ---- layers 1 + 2 fused over the 7 K blocks of layer 2, software-pipelined as in the exact kernel: the layer-1
        // MFMAs of block b + 1 are issued before the VALU epilogue of block b
        f32x4 acc2[4][NT];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc2[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // Stage b = layer-2 MFMAs of block b + layer-1 MFMAs of block b + 2 + VALU epilogue of block b + 1, see stage()
        f16x8 bhA[NT], blA[NT], bhB[NT], blB[NT];
        f32x4 acc3[4][NT];
        if constexpr (SHARED) {
            stage_sh<-1>(lds4, ldsv, lb, bhB, blB, acc2, bhA, blA);      // Hadamard + split of block 0
            SP_TICK(3); SP_TICK(4);
            stage_sh<0>(lds4, ldsv, lb, bhA, blA, acc2, bhB, blB);
            SP_TICK(5);
            stage_sh<1>(lds4, ldsv, lb, bhB, blB, acc2, bhA, blA);
            SP_TICK(6);
            stage_sh<2>(lds4, ldsv, lb, bhA, blA, acc2, bhB, blB);
            SP_TICK(7);
            stage_sh<3>(lds4, ldsv, lb, bhB, blB, acc2, bhA, blA);
            SP_TICK(8);
            stage_sh<4>(lds4, ldsv, lb, bhA, blA, acc2, bhB, blB);
            SP_TICK(9);
            stage_sh<5>(lds4, ldsv, lb, bhB, blB, acc2, bhA, blA);
            SP_TICK(10);
            tail<false>(lds4, ldsv, lb, c2 * sc.r21, sc.S2, bhA, blA, acc2, acc3, cj);
        } else {
        f32x4 accA[2][NT], accB[2][NT];
        stage<-2>(lds4, ldsv, lb, cbh, cbl, bhB, blB, acc2, accA, accB, bhB, blB, cj);      // layer-1 block 0
        SP_TICK(3);
        stage<-1>(lds4, ldsv, lb, cbh, cbl, bhB, blB, acc2, accB, accA, bhA, blA, cj);      // layer-1 block 1, epilogue of block 0
        SP_TICK(4);
        stage<0>(lds4, ldsv, lb, cbh, cbl, bhA, blA, acc2, accA, accB, bhB, blB, cj);
        SP_TICK(5);
        stage<1>(lds4, ldsv, lb, cbh, cbl, bhB, blB, acc2, accB, accA, bhA, blA, cj);
        SP_TICK(6);
        stage<2>(lds4, ldsv, lb, cbh, cbl, bhA, blA, acc2, accA, accB, bhB, blB, cj);
        SP_TICK(7);
        stage<3>(lds4, ldsv, lb, cbh, cbl, bhB, blB, acc2, accB, accA, bhA, blA, cj);
        SP_TICK(8);
        stage<4>(lds4, ldsv, lb, cbh, cbl, bhA, blA, acc2, accA, accB, bhB, blB, cj);
        SP_TICK(9);
        stage<5>(lds4, ldsv, lb, cbh, cbl, bhB, blB, acc2, accB, accA, bhA, blA, cj);
        SP_TICK(10);
        tail(lds4, ldsv, lb, c2 * sc.r21, sc.S2, bhA, blA, acc2, acc3, cj);
        if (SP_COSJOB) cj.finish(cbh, cbl);      // (register renaming: the operands of the next environment)
        }
        SP_TICK(11);
        const float c3e = c3 * sc.r32;      // layer-3 accumulators carry S2 2^k3: to S3
        float qv;
        if constexpr (!QUANT) {
            // ---- layer 3 epilogue, tau mean, f32 output layer (as in the exact kernel; the sums carry the factor S3) ---------
            float hs[16];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const f32x4 sb = ldsv[lb.fl + ((OFF_B3 - OFF_B1) >> 2) + 4 * mt] * sc.S3;
                const f32x4 h0 = relu4s(fma4(acc3[mt][0], c3e, sb)), h1 = relu4s(fma4(acc3[mt][1], c3e, sb));
#pragma unroll
                for (int r = 0; r < 4; ++r) hs[4 * mt + r] = h0[r] + h1[r];
            }
            row_sum16_x16(hs);                          // sum over the 32 taus of h3[16 mt + 4 g + r], in every lane of row group g
            float part = 0.f;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const f32x4 a = ldsv[lb.w_hi + ((OFF_W4 >> 2) - 4096) + mt * 64];
#pragma unroll
                for (int r = 0; r < 4; ++r) part = fmaf(a[r], hs[4 * mt + r], part);
            }
            part = sum_rows4(part);                     // the four row groups' shares of action `col`
            qv = part * (sc.invS3 * (1.0f / K_TAUS)) + lds[OFF_B4 + col];     // Q(s, action = col), valid for col < 9
        } else {
            // ---- quantile values Z(tau, a), written out, and their tau mean (q_quantiles)
            qv = q_quantiles(lds, ldsv, lb, acc3, c3e, sc, lane, quantiles + (size_t)e * K_TAUS * A_OUT);
        }
        if (qvals && lane < A_OUT) qvals[(size_t)e * A_OUT + lane] = qv;
        // ---- IQNAgent.act epilogue (agent.py:199-203): argmax, epsilon-greedy ------------------------
        if (actions) {
            // lane a holds action a: nine v_readlane (no LDS round trip); first maximum wins, like np.argmax
            float best = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qv), 0));
            int arg = 0;
#define SP_ARG(a) { const float v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qv), a)); if (v > best) { best = v; arg = a; } }
            SP_ARG(1) SP_ARG(2) SP_ARG(3) SP_ARG(4) SP_ARG(5) SP_ARG(6) SP_ARG(7) SP_ARG(8)
#undef SP_ARG
            if (lane == 0) {
                int act = arg;
                if (!ROWS && explore_u && eps > 0.f) {       // (a listed row is known to be greedy)
                    const float u = u_explore;               // greedy iff u > eps (agent.py:200); requested at the top of the iteration
                    if (!(u > eps)) act = explore_action(u, eps);
                }
                actions[e] = act;
            }
        }
        SP_TICK(12);
        if ((SP_ABL & 64) && blockIdx.x == 3 && wave == 1 && lane == 0 && ++sp_iter == 6)
            printf("phase cycles (block 3, wave 1, 6th env): cos %llu  encoder+scale %llu  stage-2 %llu  stage-1 %llu  stages0..5 %llu %llu %llu %llu %llu %llu  tail %llu  output %llu  | env total %llu\n",
                   tk[1] - tk[0], tk[2] - tk[1], tk[3] - tk[2], tk[4] - tk[3], tk[5] - tk[4], tk[6] - tk[5], tk[7] - tk[6], tk[8] - tk[7], tk[9] - tk[8], tk[10] - tk[9],
                   tk[11] - tk[10], tk[12] - tk[11], tk[12] - tk[0]);
#undef SP_TICK
        if constexpr (LATE) e = e_follow;
        else if constexpr (ROWS) { e = e_follow; e_follow = e_ahead; }
        else e += e_stride;
    }
