// iqn_act_exact.h -- the IQN action-value network of iqn_act.hip on the exact-f32 MFMA (variant 0): the accuracy yardstick of the split-f16 kernel.
// Included by iqn_act.hip inside its anonymous namespace, after iqn_act_common.h (uses IqnWeights, row_sum16, draw_block, the layer constants).
//
// MFMA mapping: exact-f32 v_mfma_f32_16x16x4_f32 (the reference is float32; no reduced precision).
// Every layer is computed TRANSPOSED, H^T = W . X^T: the weights are the A operand (16 output
// features x 4 k), the activations the B operand (4 k x 16 tau rows) and the C tile is
// [16 features x 16 taus] with lane l holding column (l & 15) and rows 4*(l >> 4) + r.  Because the
// k order of a dot product is free, MFMA step (t, r) of the NEXT layer is defined to consume input
// features {16t + 4g + r : g = 0..3} -- which is exactly register r of C tile t in lane group g.  So a
// layer's accumulator registers ARE the next layer's B operands: no LDS round trip, no shuffles.
// The weights are permuted into that order once per weight update (iqn_pack_kernel) and copied to LDS per workgroup
// (LDS_FLOATS floats incl. the encoders and the per-wave feature buffers, nearly all of the CU's 160 KB: one 512-thread workgroup per CU,
// 2 waves per SIMD so one wave's bias / ReLU / cos VALU work runs under the other's MFMAs); each ds_read_b128 feeds 4 k-steps x 2 tau
// tiles = 8 MFMAs.  Layers 1 and 2 are fused over the 13 feature tiles of the 208-wide activation,
// so the live state is 32 accumulator + 32 cos registers per lane.

// LDS layout (floats)
constexpr int OFF_W1 = 0;                         // [13 t][4 m4][64 lanes][4]
constexpr int OFF_W2 = OFF_W1 + T1 * 4 * 64 * 4;  // [4 mt][13 t][64][4]
constexpr int OFF_W3 = OFF_W2 + 4 * T1 * 64 * 4;  // [4 mt][4 t2][64][4]
constexpr int OFF_W4 = OFF_W3 + 4 * 4 * 64 * 4;   // [4 t2][64][4]
constexpr int OFF_B1 = OFF_W4 + 4 * 64 * 4;       // [208]
constexpr int OFF_B2 = OFF_B1 + F;                // [64]
constexpr int OFF_B3 = OFF_B2 + H;                // [64]
constexpr int OFF_B4 = OFF_B3 + H;                // [16]
constexpr int OFF_WE = OFF_B4 + 16;               // [7 i4][208 f][4]: block-diagonal encoder weights
constexpr int OFF_BE = OFF_WE + OBS4 * F * 4;     // [208] encoder biases
constexpr int OFF_FB = OFF_BE + F;                // [8 waves][208] per-wave feature buffer
constexpr int LDS_FLOATS = OFF_FB + 8 * F;
static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS image of the exact-f32 act kernel must fit the CU's 160 KB");

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ f32x4 relu4(f32x4 v) {
    f32x4 r;
    r.x = v.x > 0.f ? v.x : 0.f; r.y = v.y > 0.f ? v.y : 0.f; r.z = v.z > 0.f ? v.z : 0.f; r.w = v.w > 0.f ? v.w : 0.f;
    return r;
}

// block-diagonal encoder weight: feature f (0..207) x observation input i (0..25)  (model.py:126-128,170-173)
__device__ __forceinline__ float enc_weight(const IqnWeights &w, int f, int i) {
    if (f < 16) return (i < 2) ? w.ve_w[f * 2 + i] : 0.f;
    if (f < 32) return (i >= 2 && i < 4) ? w.ge_w[(f - 16) * 2 + (i - 2)] : 0.f;
    return (i >= 4 && i < OBS) ? w.se_w[(f - 32) * 22 + (i - 4)] : 0.f;
}

// Value of element i of the LDS weight image (floats [0, OFF_FB)): weights permuted into MFMA A-fragment
// order (nn.Linear stores [out][in]), biases, block-diagonal encoder.
__device__ __forceinline__ float pack_element(const IqnWeights &w, int i) {
    if (i < OFF_B1) {
        const int j = i & 3, l = (i >> 2) & 63, g = l >> 4, row = l & 15;
        if (i < OFF_W2) {            // W1p[t][m4][l][j] = W1[16t + row][4*(4*m4 + j) + g]
            const int q = i >> 8, m4 = q & 3, t = q >> 2;
            return w.W1[(16 * t + row) * N_COS + 4 * (4 * m4 + j) + g];
        } else if (i < OFF_W3) {     // W2p[mt][t][l][r] = W2[16mt + row][16t + 4g + r]
            const int q = (i - OFF_W2) >> 8, t = q % T1, mt = q / T1;
            return w.W2[(16 * mt + row) * F + 16 * t + 4 * g + j];
        } else if (i < OFF_W4) {     // W3p[mt][t2][l][r] = W3[16mt + row][16t2 + 4g + r]
            const int q = (i - OFF_W3) >> 8, t2 = q & 3, mt = q >> 2;
            return w.W3[(16 * mt + row) * H + 16 * t2 + 4 * g + j];
        }                            // W4p[t2][l][r] = W4[row][16t2 + 4g + r] (rows >= 9 are zero)
        const int t2 = (i - OFF_W4) >> 8;
        return row < A_OUT ? w.W4[row * H + 16 * t2 + 4 * g + j] : 0.f;
    }
    if (i < OFF_B2) return w.b1[i - OFF_B1];
    if (i < OFF_B3) return w.b2[i - OFF_B2];
    if (i < OFF_B4) return w.b3[i - OFF_B3];
    if (i < OFF_WE) return (i - OFF_B4) < A_OUT ? w.b4[i - OFF_B4] : 0.f;
    if (i < OFF_BE) {                // WEp[i4][f][c] = Wenc[f][4*i4 + c] (block-diagonal 208 x 26, zero elsewhere / padding)
        const int k = i - OFF_WE, c = k & 3, f = (k >> 2) % F, i4 = (k >> 2) / F;
        const int inp = 4 * i4 + c;
        return inp < OBS ? enc_weight(w, f, inp) : 0.f;
    }
    const int f = i - OFF_BE;
    return f < 16 ? w.ve_b[f] : (f < 32 ? w.ge_b[f - 16] : w.se_b[f - 32]);
}

// Builds the LDS image (OFF_FB floats) once per weight update in global memory, so that each workgroup of the
// act kernel fills its LDS with a straight 16-byte coalesced copy instead of a 38 K-element gather.
__global__ __launch_bounds__(256) void iqn_pack_kernel(IqnWeights w, float *__restrict__ packed) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < OFF_FB) packed[i] = pack_element(w, i);
}

constexpr int PACK_BLOCKS = (OFF_FB + 255) / 256;

// The same weight image PLUS the random numbers of the call in one launch: blocks [0, PACK_BLOCKS) pack, the others
// fill draws[0 .. 32 n) with tau = U[0,1) * cvar (model.py:149-153; per-row cvar if cvar_row) and draws[32 n .. 33 n)
// with the exploration uniforms of IQNAgent.act (agent.py:199).  rng_state = {seed, call counter}; the counter is
// advanced by the act kernel that follows in the stream.
__global__ __launch_bounds__(256) void iqn_prep_kernel(IqnWeights w, float *__restrict__ packed, const uint64_t *__restrict__ rng_state,
                                                       float *__restrict__ draws, int n, const float *__restrict__ cvar_row,
                                                       float cvar, int pack_blocks) {
    // pack_blocks = PACK_BLOCKS when the cached weight image is stale (mn_iqn_weights_changed), else 0
    if ((int)blockIdx.x < pack_blocks) {
        const int i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i < OFF_FB) packed[i] = pack_element(w, i);
        return;
    }
    draw_block(rng_state, draws, n, cvar_row, cvar, pack_blocks);
}

// QUANT = false: the training / acting hot path (tau-mean before the linear output layer, 960 MFMAs per env).
// QUANT = true : IQNAgent.act_eval (agent.py:217-236): the output layer runs per tau on the matrix pipe (+32 MFMAs on a
//                padded 16-row tile), the [n][32][9] quantile values are written out and Q is their mean.
template <bool QUANT>
__global__ __launch_bounds__(512, 2) void iqn_qvals_kernel(const float *__restrict__ obs, const float *__restrict__ taus,
                                                           const float *__restrict__ packed, float *__restrict__ qvals,
                                                           const float *__restrict__ explore_u, float eps,
                                                           int32_t *__restrict__ actions, int n,
                                                           uint64_t *__restrict__ rng_state, float *__restrict__ quantiles) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    if (rng_state && blockIdx.x == 0 && tid == 0) rng_state[1] += 1;   // the draws of this call were made by iqn_prep_kernel
    {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(packed);
        f32x4 *dst = reinterpret_cast<f32x4 *>(lds);
        for (int i = tid; i < OFF_FB / 4; i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();

    const int lane = tid & 63, g = lane >> 4, col = lane & 15;
    const int wave = tid >> 6, waves_per_block = blockDim.x >> 6;
    const f32x4 *ldsv = reinterpret_cast<const f32x4 *>(lds);

    // cos(tau * pi * k) = cos(2 pi * (tau * k / 2)), k = 4m + g: the phase in REVOLUTIONS is tau * (k/2),
    // one exact-ish multiply; v_fract + v_cos_f32 replace libm's ~35-instruction range reduction.  The
    // reference rounds tau * float32(pi k) before its cos (model.py:130,155), so the two already
    // differ by ~1e-5 rad of input rounding at k = 63; that noise dominates either cos error.
    float hk[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) hk[m] = 0.5f * (float)(4 * m + g);

    // one environment (32 tau rows = NT = 2 column tiles) per wave iteration
    constexpr int NT = 2;
    for (int e = blockIdx.x * waves_per_block + wave; e < n; e += gridDim.x * waves_per_block) {
        float tau[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) tau[nt] = taus[(size_t)e * K_TAUS + 16 * nt + col];
        // layer-1 B operands: cos(tau * pis[k]) for k = 4m + g  (model.py:155)
        float cb[16][NT];
#pragma unroll
        for (int m = 0; m < 16; ++m)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) cb[m][nt] = __builtin_amdgcn_cosf(__builtin_amdgcn_fractf(tau[nt] * hk[m]));

        // ---- observation encoders (model.py:170-173): lane l computes features l, l+64, l+128, l+192 from
        // the 26 inputs (wave-uniform -> scalar loads) and parks them in this wave's LDS buffer, from
        // where every lane later reads the float4 {16t + 4g + r} it needs for the Hadamard product
        {
            const float *orow = obs + (size_t)__builtin_amdgcn_readfirstlane(e) * OBS;
            float ov[OBS4 * 4];
#pragma unroll
            for (int i = 0; i < OBS4 * 4; ++i) ov[i] = i < OBS ? orow[i] : 0.f;
            float *fb = lds + OFF_FB + wave * F;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = lane + 64 * j;
                if (f < F) {
                    float a = lds[OFF_BE + f];
#pragma unroll
                    for (int i4 = 0; i4 < OBS4; ++i4) {
                        const f32x4 wv = ldsv[(OFF_WE >> 2) + i4 * F + f];
                        a += wv[0] * ov[4 * i4] + wv[1] * ov[4 * i4 + 1] + wv[2] * ov[4 * i4 + 2] + wv[3] * ov[4 * i4 + 3];
                    }
                    fb[f] = a;
                }
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        const f32x4 *fbv = reinterpret_cast<const f32x4 *>(lds + OFF_FB + wave * F) + g;   // + 4*t per tile

        f32x4 acc2[4][NT];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc2[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

        // ---- layers 1 + 2 fused over the 13 feature tiles, software-pipelined: the layer-1 MFMAs of
        // tile t+1 are issued BEFORE the bias / ReLU / Hadamard epilogue of tile t, so the wave's own VALU
        // work sits in the shadow of its own MFMAs (in-order issue would otherwise drain the matrix pipe
        // at every tile boundary) -------------------------------------------------------------------
        f32x4 acc1[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc1[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m4 = 0; m4 < 4; ++m4) {
            const f32x4 a = ldsv[(OFF_W1 >> 2) + m4 * 64 + lane];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc1[nt] = mfma(a[j], cb[4 * m4 + j][nt], acc1[nt]);
        }
#pragma unroll
        for (int t = 0; t < T1; ++t) {
            f32x4 nxt[NT];
            if (t + 1 < T1) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) nxt[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int m4 = 0; m4 < 4; ++m4) {
                    const f32x4 a = ldsv[(OFF_W1 >> 2) + ((t + 1) * 4 + m4) * 64 + lane];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) nxt[nt] = mfma(a[j], cb[4 * m4 + j][nt], nxt[nt]);
                }
            }
            const f32x4 fv = fbv[4 * t];                             // features[e][16t + 4g + r]
            const f32x4 bias = ldsv[(OFF_B1 >> 2) + 4 * t + g];      // b1[16t + 4g + r]
            f32x4 h1[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) h1[nt] = relu4(acc1[nt] + bias) * fv;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const f32x4 a = ldsv[(OFF_W2 >> 2) + (mt * T1 + t) * 64 + lane];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc2[mt][nt] = mfma(a[r], h1[nt][r], acc2[mt][nt]);
            }
            if (t + 1 < T1) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc1[nt] = nxt[nt];
            }
        }
        // ---- layer 2 epilogue, layer 3 ---------------------------------------------------------------
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const f32x4 bias = ldsv[(OFF_B2 >> 2) + 4 * mt + g];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc2[mt][nt] = relu4(acc2[mt][nt] + bias);
        }
        f32x4 acc3[4][NT];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc3[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t2 = 0; t2 < 4; ++t2) {
                const f32x4 a = ldsv[(OFF_W3 >> 2) + (mt * 4 + t2) * 64 + lane];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc3[mt][nt] = mfma(a[r], acc2[t2][nt][r], acc3[mt][nt]);
            }
            const f32x4 bias = ldsv[(OFF_B3 >> 2) + 4 * mt + g];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc3[mt][nt] = relu4(acc3[mt][nt] + bias);
        }
        // ---- layer 4 + mean over the 32 taus (model.py:185,190).  The output layer is linear, so
        // mean_tau(W4 h3(tau) + b4) = W4 mean_tau(h3(tau)) + b4: the tau mean is taken FIRST (DPP row sums of the
        // layer-3 accumulators) and the 9 x 64 output layer becomes one small VALU mat-vec per environment
        // instead of 32 MFMAs on a padded 16-row tile (3 % of the kernel's matrix work).
        // After row_sum16 every lane of row group g holds sum_tau h3[16mt + 4g + r]; lane (g, col) then forms the
        // part of action `col` that comes from its 16 features (W4p[mt][lane][r] = W4[col][16mt + 4g + r], zero rows
        // for col >= 9) and the four row groups are added with two cross-row shuffles.
        float qv;
        if constexpr (!QUANT) {
            float part = 0.f;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const f32x4 a = ldsv[(OFF_W4 >> 2) + mt * 64 + lane];
#pragma unroll
                for (int r = 0; r < 4; ++r) part = fmaf(a[r], row_sum16(acc3[mt][0][r] + acc3[mt][1][r]), part);
            }
            part += __shfl_xor(part, 16);
            part += __shfl_xor(part, 32);
            qv = part * (1.0f / K_TAUS) + lds[OFF_B4 + col];     // Q(s, action = col), valid for col < 9
        } else {
            // quantile values Z(tau, a) = W4 h3(tau) + b4 (model.py:185): C tile [16 padded actions x 16 taus] per tau tile;
            // lane (g, col) holds actions 4g + r of tau 16 nt + col
            f32x4 acc4[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc4[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t2 = 0; t2 < 4; ++t2) {
                const f32x4 a = ldsv[(OFF_W4 >> 2) + t2 * 64 + lane];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc4[nt] = mfma(a[r], acc3[t2][nt][r], acc4[nt]);
            }
            const f32x4 b4 = ldsv[(OFF_B4 >> 2) + g];
            float mine = 0.f;      // lane `a` (< 9) ends up with Q(s, a) = mean over the 32 taus
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a_idx = 4 * g + r;
                float sum = 0.f;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const float z = acc4[nt][r] + b4[r];
                    if (a_idx < A_OUT) quantiles[((size_t)e * K_TAUS + 16 * nt + col) * A_OUT + a_idx] = z;
                    sum += z;
                }
                sum = row_sum16(sum);                    // over the 16 tau columns of the row group
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) {         // hand action 4 gg + r to lane (4 gg + r)
                    const float v = __shfl(sum, 16 * gg);
                    if (lane == 4 * gg + r) mine = v;
                }
            }
            qv = mine * (1.0f / K_TAUS);
        }
        if (qvals && lane < A_OUT) qvals[(size_t)e * A_OUT + lane] = qv;
        // ---- IQNAgent.act epilogue (agent.py:199-203): argmax, epsilon-greedy ------------------------
        if (actions) {
            // lane a holds action a; gather the 9 values (first maximum wins, like np.argmax)
            float best = -INFINITY;
            int arg = 0;
#pragma unroll
            for (int a = 0; a < A_OUT; ++a) {
                const float v = __shfl(qv, a);
                if (v > best) { best = v; arg = a; }
            }
            if (lane == 0) {
                int act = arg;
                if (explore_u && eps > 0.f) {
                    const float u = explore_u[e];            // greedy iff u > eps (agent.py:200)
                    if (!(u > eps)) { act = (int)(u / eps * (float)A_OUT); act = act > A_OUT - 1 ? A_OUT - 1 : act; }
                }
                actions[e] = act;
            }
        }
    }
}
