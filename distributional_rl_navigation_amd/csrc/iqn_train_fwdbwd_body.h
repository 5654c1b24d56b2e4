// iqn_train_fwdbwd_body.h -- the statements of one forward / backward workgroup of the IQN gradient step (csrc/iqn_train.hip), included INSIDE the kernels that
// run them: iqn_train_fwdbwd<XCHG, FUSED>, iqn_group_fwdbwd_kernel, iqn_per_fwdbwd_kernel, iqn_munch_fwdbwd_kernel and iqn_rule_fwdbwd_kernel<RULE>.  Expects in scope: `args` (const TrainArgs: the launch's arguments), the
// compile-time constants XCHG, FUSED, PER (the weighted step of prioritized replay: `per_weights` [batch] scales each element's loss terms, `per_absdelta` [batch]
// receives its mean |TD error|; both are named, and NULL, where PER is false) and MUNCH (the Munchausen target, marinenav_hip.h: `munch` -- a MunchArgs: the third tau
// set [batch][8], alpha, the entropy temperature, the clip bound and the optional targets_out [batch][8] -- is named, and all zero, where MUNCH is false; a MUNCH kernel
// is launched local-only with a given batch) and RULE (0: the per-sample max; RULE_MEAN / RULE_DOUBLE: the greedy-on-mean targets, marinenav_hip.h "Target rules":
// `rule` -- a RuleArgs: the third tau set [batch][8] of RULE_DOUBLE and the optional targets_out [batch][8] and select_out [batch] -- is named, and all zero, where
// RULE is 0; launched as a MUNCH kernel is), blockIdx.x = the workgroup's index in its learner's launch, and everything iqn_train.hip defines in front of its kernels.
// No include guard: it is a function body, included once per kernel.
    extern __shared__ __align__(16) float S[];
    __shared__ int s_act[BE];
    __shared__ int s_got;
    // ---- the counters this launch starts from; nothing in memory moves before its last step's reduction + Adam blocks have all taken their ticket
    uint64_t epoch0, rs0 = 0, rs1 = 0, tg0 = 0, tg1 = 0;      // scalar state first (generator state, staging tag): issued before the weight requests flood the memory pipeline
    int32_t step0 = 0;
    {
        const int n_part = args.batch / BE;
        epoch0 = *reinterpret_cast<const uint64_t *>(args.ws + ws_epoch(n_part));
        if (args.ba.rng_state) {
            const uint64_t *stg_tag = reinterpret_cast<const uint64_t *>(args.ws + ws_epoch(n_part) + 4);
            rs0 = args.ba.rng_state[0]; rs1 = args.ba.rng_state[1];
            tg0 = stg_tag[0]; tg1 = stg_tag[1];
        }
        if (FUSED) step0 = *args.tail.step;
    }
#ifdef MN_TRAIN_PHASES
    if (tid_now() == 0) g_wgt[blockIdx.x][0] = wall_clock64();
#endif

    // Iteration 0: the forward / backward pass (target workgroups: the target forward pass); iteration 1 (fused step): target and extra workgroups run the reduction + Adam role.
    for (int k = 0; k <= (FUSED ? 1 : 0); ++k) {
    // (One step's scalar and address arithmetic must not be hoisted out of the loop -- hundreds of values would then live across the whole body: the thread index is
    // opaque at every use (tid_now), the block index and the kernel arguments -- re-read from the kernarg segment -- are made opaque per iteration, and everything
    // derived from them, the workgroup's role included, is derived again.)
    const int tid = tid_now();
    TrainArgsK A = (TrainArgsK)__builtin_amdgcn_kernarg_segment_ptr();
    int bid = blockIdx.x;
    if (FUSED) asm volatile("" : "+s"(A), "+s"(bid));
    const BatchArgs ba = FUSED ? ld_batch_args(A) : args.ba;
    const StepTail tail = FUSED ? ld_step_tail(A) : args.tail;
    float *const ws = FUSED ? A->ws : args.ws;
    const float *const PL = FUSED ? A->PL : args.PL, *const PT = FUSED ? A->PT : args.PT;
    const int batch = FUSED ? A->batch : args.batch, mode = FUSED ? A->mode : args.mode;
    const int n_part = batch / BE;
    const bool two_roles = mode == MODE_TWO_ROLES;      // (FUSED: always)
    const int n_fwd = two_roles ? 2 * n_part : n_part;
    const bool is_extra = FUSED && bid >= n_fwd;            // reduction + Adam blocks only
    const bool is_target = two_roles && bid < n_part;       // target workgroups come FIRST in dispatch order: nothing they need is produced by a local workgroup
    const int part = is_extra ? 0 : (two_roles && !is_target ? bid - n_part : bid);
    const int b0 = part * BE;
    const int pb = is_extra ? n_part + (bid - n_fwd) : bid, n_phys = n_part + tail.n_extra;      // reduction + Adam role: physical block pb of n_phys
#ifdef MN_TRAIN_PHASES
    const int ph_local = two_roles ? n_part : 0;
#else
    const int ph_local = -1;
#endif
    PH(0);
    const float gamma = FUSED ? A->gamma : args.gamma;
    const int use_staged = FUSED ? A->use_staged : args.use_staged;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, i = lane & 15, g = lane >> 4;
    const ParamView VL(PL);
    const float *stage = ws + ws_stage(n_part);
    const int st_slot = min(tid / STG, BE - 1), st_e = tid % STG;
    float *out = ws + (size_t)part * P_PAD;
    const __amdgpu_buffer_rsrc_t out_rsrc = __builtin_amdgcn_make_buffer_rsrc(out, 0, P_PAD * 4, 0x00020000);
    if (k < 1 && !is_extra) {
    // hand-off tag of this step: never 0 (the workspace starts zero-filled), different from the neighbouring steps' and launches' tags
    const uint32_t tag = (uint32_t)((epoch0 + (uint64_t)k) % 0xFFFFFFFFull) + 1u;
    gu64 *granules = (gu64 *)(ws + ws_tdq(n_part)) + (size_t)part * ROWS;
    if (FUSED && !is_target && tid == 0) {      // where this local workgroup runs (see "local workgroup" below)
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        __hip_atomic_store((gu64 *)(ws + ws_xcc(n_part)) + part, ((uint64_t)tag << 32) | (uint64_t)(xcc & 15u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

    // ---- The first requests of a step: (a) -- first step of a launch -- this workgroup's two batch slots as the previous launch's reduction blocks STAGED them
    // (transitions and taus, 72 floats per slot, at an address that depends on nothing but the kernel arguments), (b) every weight
    // operand of the forward pass.  One round trip instead of three dependent ones (generator state -> ring rows -> transitions).
    // (Measured and dropped: gathering the batch in FRONT of that wait -- 1.6 us earlier requests, but two sites that define the 140 weight registers cost 48 bytes of
    // scratch per lane and the step got 1 us longer.)
    const bool try_staged = use_staged && k == 0;
    float st_v = 0.f;
    if (try_staged) st_v = stage[(b0 + st_slot) * STG + st_e];      // kernel argument: a scalar branch
    FwdWeights w;
    const ParamView V(is_target ? PT : PL);
    prefetch_forward(w, V);
    PH(14);  /* all requests issued */
    // the staged batch is this step's batch iff it was drawn for this call counter from a ring of this many rows
    uint64_t base = 0;
    bool staged = false;
    if (ba.rng_state) {
        base = mix64(rs0 + 0x9E3779B97F4A7C15ull * (rs1 + (uint64_t)k + 1));      // = sample_base of the generator at call counter rs1 + k
        staged = try_staged && tg0 == rs1 && tg1 == (uint64_t)ba.ring_n;
    }
    PH(15);  /* generator state / staging tag read */
    int64_t row0 = 0, row1 = 0;      // (BE = 2; selects instead of an indexed array, which would live in scratch)
    if (staged) {      // uniform
        if (tid < BE * STG) {
            const int o = st_slot * 28;
            if (st_e < OBS) { if (!is_target) S[S_OBS + o + st_e] = st_v; }
            else if (st_e < 2 * OBS) { if (is_target) S[S_OBS + o + st_e - OBS] = st_v; else if (!two_roles) S[T_OBS + o + st_e - OBS] = st_v; }
            else if (st_e == 2 * OBS) s_act[st_slot] = (int)st_v;
            else if (st_e == 2 * OBS + 1) S[S_MISC + st_slot] = st_v;
            else if (st_e == 2 * OBS + 2) S[S_MISC + BE + st_slot] = st_v;
            else if (st_e >= 56 && st_e < 64) { if (is_target) S[S_TAU + st_slot * NQ + st_e - 56] = st_v; else if (!two_roles) S[T_TAU + st_slot * NQ + st_e - 56] = st_v; }
            else if (st_e >= 64) { if (!is_target) S[S_TAU + st_slot * NQ + st_e - 64] = st_v; }
        }
    } else {
        // ---- no (valid) staged batch: the batch rows of this workgroup (scalar arithmetic, or two loads in the given-batch form) ...
        float tau_t = 0.f, tau_l = 0.f;
        const int e_t = b0 * NQ + (tid & (ROWS - 1));
        if (ba.rng_state) {
            row0 = perm_row(base, (uint32_t)ba.ring_n, (uint32_t)b0);
            row1 = perm_row(base, (uint32_t)ba.ring_n, (uint32_t)(b0 + 1));
            // taus: target draws first (model.py:149 is called for the target network first, agent.py:279-286)
            tau_t = sample_tau(base, e_t);
            tau_l = sample_tau(base, batch * NQ + e_t);
        } else {
            row0 = ba.idx[b0];
            row1 = ba.idx[b0 + 1];
            tau_t = ba.taus_t[e_t];
            tau_l = ba.taus_l[e_t];
        }
        float tau_m = 0.f;      // MUNCH: the third tau set, for the target network's pass over the CURRENT state
        if (MUNCH) tau_m = munch.taus[e_t];
        if (RULE == RULE_DOUBLE) tau_m = rule.taus[e_t];      // the third tau set, for the LOCAL network's selecting pass over the NEXT state
        // ---- ... then the transitions, in one straight line without branches (all threads load, clamped -- the few that matter
        // store to LDS below)
        const int g_be = (tid / OBS) & 1, g_k = tid % OBS;
        const int64_t g_row = g_be ? row1 : row0, m_row = (tid & 1) ? row1 : row0;
        const float g_obs = (is_target ? ba.ring_ns : ba.ring_s)[g_row * OBS + g_k];
        const float g_tobs = ba.ring_ns[g_row * OBS + g_k];          // only kept when this workgroup runs both networks
        const int g_act = (int)ba.ring_a[m_row];
        const float g_rew = ba.ring_r[m_row], g_done = ba.ring_d[m_row];
        if (tid < ROWS) {
            S[S_TAU + tid] = is_target ? tau_t : tau_l;
            if (!two_roles) S[T_TAU + tid] = tau_t;
            if (MUNCH || RULE == RULE_DOUBLE) S[S_QT + tid] = tau_m;      // (the TD targets' slots, which nothing writes before both target passes are over)
        }
        // gathered transitions -> LDS (replay_buffer.py:42-57)
        if (tid < BE * OBS) {
            S[S_OBS + g_be * 28 + g_k] = g_obs;
            if (!two_roles) S[T_OBS + g_be * 28 + g_k] = g_tobs;
        }
        if (tid < BE) {
            s_act[tid] = g_act;
            S[S_MISC + tid] = g_rew;
            S[S_MISC + BE + tid] = g_done;
        }
    }
    PH(16);  /* wave 0 has its transitions in LDS */
    __syncthreads();
    prefetch_forward_late(w, V);
    PH(1);   /* draw + gather + weight requests */

    // output-layer row of the action taken, for dh3 (element tid + 512 e of the [16][64] tile: row 8 e + (tid >> 6), column tid & 63,
    // i.e. batch element e): two more early requests
    float w4row[2] = {0.f, 0.f};
    if (!is_target) {
#pragma unroll
        for (int e = 0; e < 2; ++e) w4row[e] = VL.f1(O_W4 + s_act[e] * H + (tid & 63));
    }
    float per_w[2] = {1.f, 1.f};      // PER: the importance weights of this workgroup's two elements, requested early like the row above
    if (PER) { per_w[0] = per_weights[b0]; per_w[1] = per_weights[b0 + 1]; }
    const PassBufs Bl = {S + S_C, is_target ? nullptr : S + S_H1, S + S_X, S + S_H2, S + S_H3, S + S_FEAT, S + S_Q};
    BwdWeights bw;
    if (is_target) forward_pass<false>(Bl, w, S + S_OBS, S + S_TAU, nullptr, VL, ph_local);
    else forward_pass<true>(Bl, w, S + S_OBS, S + S_TAU, &bw, VL, ph_local);

    if (is_target) {
        // publish the 16 TD targets: one self-tagged 8-byte granule each ({epoch, value}, agent-scope store: the data is the flag)
        if (tid < ROWS) {
            const int be = tid >> 3;
            const float v = td_target(S + S_Q, tid, S[S_MISC + be], S[S_MISC + BE + be], gamma);
            __hip_atomic_store(granules + tid, ((uint64_t)tag << 32) | (uint64_t)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        PH(7);   /* granules published */
        if (bid == 0) write_batch_copies(ba, base, batch);
#ifdef MN_TRAIN_PHASES
        if (tid_now() == 0) g_wgt[blockIdx.x][1] = wall_clock64();
#endif
    } else {

    // ---- local workgroup
    // The rows w = x (mod 8) are summed inside one XCD's L2, so their workgroups have to share an XCD.  The dispatcher deals
    // workgroups out to the XCDs round-robin (scripts/probes/xcc_placement.hip) -- from XCD 0 in a fresh process, from another one after other streams were
    // in use -- so block index % 8 names a set of workgroups on ONE XCD, not which.  Each local workgroup publishes the XCD it runs on; a group's XCD is
    // that of its first workgroup, whose word the others read here (long before they need it, behind the TD targets).
    uint64_t lead_word = 0;
    unsigned my_xcc = 0;
    if (FUSED) {
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(my_xcc));
        my_xcc &= 15u;
        if (tid == 0 && (part >> 3) != 0) lead_word = __hip_atomic_load((const gu64 *)(ws + ws_xcc(n_part)) + (part & 7), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // ---- TD targets: from the target workgroup of the same two batch elements (ready by now -- it ran the same forward at the same
    // time on another CU), or computed here (mode 1; or the granules did not arrive within the bound, which in-order workgroup
    // dispatch makes impossible -- kept so that a wait can never hang the device)
    if (two_roles) {
        if (wave == 0) {
            bool ok = false;
            float v = 0.f;
            const uint64_t t0 = __builtin_readcyclecounter();
            for (;;) {
                uint64_t x = (uint64_t)tag << 32;
                if (lane < ROWS) x = __hip_atomic_load(granules + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = (uint32_t)(x >> 32) == tag;
                v = __uint_as_float((uint32_t)x);
                if (__all(ok)) break;
                if (__builtin_readcyclecounter() - t0 > 400000000ull) break;      // ~0.2 s of shader clocks
                __builtin_amdgcn_s_sleep(2);
            }
            const bool all_ok = __all(ok);
            if (all_ok && lane < ROWS) S[S_QT + lane] = v;
            if (lane == 0) s_got = all_ok ? 1 : 0;
            if (!all_ok && lane == 0) atomicAdd(reinterpret_cast<unsigned *>(ws + ws_epoch(n_part) + 13), 1u);      // (diagnostic: TD targets computed here after a wait in vain)
        }
        __syncthreads();
    }
    if (!two_roles || !s_got) {
        if (two_roles) {   // late fallback: the target side's inputs, from the staged slots or gathered now
            const int be = min(tid / OBS, BE - 1), kk = tid % OBS;
            if (staged) {
                if (tid < BE * OBS) S[T_OBS + be * 28 + kk] = stage[(b0 + be) * STG + OBS + kk];
                if (tid < ROWS) S[T_TAU + tid] = stage[(b0 + (tid >> 3)) * STG + 56 + (tid & 7)];
            } else {
                if (tid < BE * OBS) S[T_OBS + be * 28 + kk] = ba.ring_ns[(be ? row1 : row0) * OBS + kk];
                if (tid < ROWS) {
                    const int e_t = b0 * NQ + tid;
                    S[T_TAU + tid] = ba.rng_state ? sample_tau(base, e_t) : ba.taus_t[e_t];
                }
            }
            __syncthreads();
        }
        FwdWeights wt;
        const ParamView VT(PT);
        if (RULE == RULE_DOUBLE) {
            // the selecting pass: the LOCAL weights on the NEXT states (the target role's observations, the third tau set) through the same T_* buffers and weight
            // registers; what survives is the two chosen actions, as bits in slots of S_G that the loss phase writes only later.  Then the registers are
            // re-requested from the target's parameters
            prefetch_forward(wt, VL);
            prefetch_forward_late(wt, VL);
            const PassBufs Bs = {S + T_C, nullptr, S + T_X, S + T_H2, S + T_H3, S + T_FEAT, S + T_Q};
            forward_pass<false>(Bs, wt, S + T_OBS, S + S_QT, nullptr, VL, -2);
            if (tid < BE) S[S_G + tid] = __int_as_float(rule_choice(S + T_Q, tid));
        }
        prefetch_forward(wt, VT);
        prefetch_forward_late(wt, VT);
        const PassBufs Bt = {S + T_C, nullptr, S + T_X, S + T_H2, S + T_H3, S + T_FEAT, S + T_Q};
        if (MUNCH) {
            // the target network on the CURRENT states (the local role's observations, the third tau set) through the same T_* buffers and weight registers; what
            // survives into the second pass is the two bonuses, in slots of S_G that the loss phase writes only later
            forward_pass<false>(Bt, wt, S + S_OBS, S + S_QT, nullptr, VT, -2);
            if (tid < BE) S[S_G + tid] = munch_bonus(S + T_Q, tid, s_act[tid], munch.alpha, munch.entropy_tau, munch.clip_lo);
        }
        forward_pass<false>(Bt, wt, S + T_OBS, S + T_TAU, nullptr, VT, -2);
        if (tid < ROWS) {
            const int be = tid >> 3;
            if (MUNCH) {
                const float y = munch_target(S + T_Q, tid, S[S_MISC + be], S[S_MISC + BE + be], gamma, munch.entropy_tau, S[S_G + be]);
                S[S_QT + tid] = y;
                if (munch.targets_out) munch.targets_out[b0 * NQ + tid] = y;
            } else if (RULE) {
                const int a_star = RULE == RULE_DOUBLE ? __float_as_int(S[S_G + be]) : rule_choice(S + T_Q, be);
                const float y = rule_target(S + T_Q, tid, a_star, S[S_MISC + be], S[S_MISC + BE + be], gamma);
                S[S_QT + tid] = y;
                if (rule.targets_out) rule.targets_out[b0 * NQ + tid] = y;
                if (rule.select_out && (tid & (NQ - 1)) == 0) rule.select_out[b0 + be] = a_star;
            } else
                S[S_QT + tid] = td_target(S + T_Q, tid, S[S_MISC + be], S[S_MISC + BE + be], gamma);
        }
        __syncthreads();
    }

    PH(8);   /* TD targets in LDS (hand-off wait, or own target forward) */
    // ---- quantile-Huber loss and dL/dQ_expected (agent.py:289-295, 401-407); every thread evaluates the (cheap) gradient of
    // the row its dh3 elements belong to, so the loss phase and the output-layer backward share one barrier interval
    // Fused step: the row is read by the workgroups of its group (block index % 8), which share an XCD, through that XCD's L2: ordinary stores.  A workgroup
    // that is NOT on its group's XCD (never observed) writes its row through to memory.
    bool wellplaced = false;
    if (FUSED) {
        __shared__ int s_well;
        if (tid == 0) {
            const gu64 *lw = (const gu64 *)(ws + ws_xcc(n_part)) + (part & 7);
            bool well = (part >> 3) == 0;      // the group's first workgroup is where the group is
            if (!well) {
                const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
                while ((uint32_t)(lead_word >> 32) != tag && __builtin_amdgcn_s_memrealtime() - t0 < 100000ull)      // (1 ms; then: not with the group)
                    lead_word = __hip_atomic_load(lw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                well = (uint32_t)(lead_word >> 32) == tag && (unsigned)(lead_word & 15u) == my_xcc;
            }
            const int gi = part >> 3;
            if (tail.misplace == 1 && gi % 5 == 0 && gi) well = false;
            if ((tail.misplace == 2 && gi) || (tail.misplace == 3 && (part & 7) == 3 && gi)) well = false;
            s_well = well ? 1 : 0;
        }
        __syncthreads();
        wellplaced = s_well != 0;
    }
    if (FUSED && !wellplaced && tid == 0)      // epoch block word [9]: local workgroups that found themselves on another XCD, ever (diagnostic)
        __hip_atomic_fetch_add(reinterpret_cast<unsigned *>(ws + ws_epoch(n_part) + 9), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool wt = FUSED && !wellplaced;
    const bool keep = FUSED && wellplaced;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int t = tid + THREADS * e, r = t >> 6, kq = t & 63, be = r >> 3;
        const float qe = S[S_Q + r * 12 + s_act[be]], tau = S[S_TAU + r];
        float lsum = 0.f, gsum = 0.f, asum = 0.f;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const float td = S[S_QT + be * NQ + j] - qe, ad = fabsf(td);
            const float hub = ad <= 1.f ? 0.5f * td * td : ad - 0.5f;
            const float wq = fabsf(tau - (td < 0.f ? 1.f : 0.f));
            lsum = fmaf(wq, hub, lsum);
            gsum = fmaf(wq, fminf(fmaxf(td, -1.f), 1.f), gsum);
            if (PER) asum = asum + ad;
        }
        const float scale = PER ? per_w[e] * (1.f / (float)(batch * NQ)) : 1.f / (float)(batch * NQ);      // (row r belongs to element r >> 3 = e)
        const float gr = -gsum * scale;
        if (kq == 0) {
            S[S_G + r] = gr;
            S[S_MISC + 2 * BE + r] = lsum * scale;
            if (PER) S[T_TAU + r] = asum;      // (the target pass's taus, which nothing reads any more: PER workgroups always run that pass themselves)
        }
        // output layer backward: only the taken action's row carries gradient
        S[S_DH3 + r * LDC + kq] = S[S_H3 + r * LDC + kq] > 0.f ? gr * w4row[e] : 0.f;
    }
    __syncthreads();
    PH(9);   /* loss + dh3 */
    if (tid == 0) {
        float l = 0.f;
        for (int r = 0; r < ROWS; ++r) l += S[S_MISC + 2 * BE + r];
        if (FUSED)      // self-tagged, polled by reduction + Adam block 0
            __hip_atomic_store((gu64 *)(ws + ws_lossq(n_part)) + part, ((uint64_t)tag << 32) | (uint64_t)__float_as_uint(l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else ws[ws_loss(n_part) + part] = l;
        if (PER) {      // the elements' new priorities: mean |TD error| over the 8 x 8 tau pairs, the 8 row sums in index order
#pragma unroll
            for (int be = 0; be < BE; ++be) {
                float d = 0.f;
                for (int q = 0; q < NQ; ++q) d = d + S[T_TAU + be * NQ + q];
                per_absdelta[b0 + be] = d * (1.f / (float)(NQ * NQ));
            }
        }
    }

    // ---- backward (all 8 waves)
    if (wave < 4) {   // dh2 = (dh3 W3) * [h2 > 0]
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = mma_a_lds<4>(S + S_DH3, LDC, bw.w3t, acc);
        const int c = wave * 16 + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rr = 4 * g + r;
            S[S_DH2 + rr * LDC + c] = S[S_H2 + rr * LDC + c] > 0.f ? acc[r] : 0.f;
        }
    } else {
        // dW3 = dh3^T h2 : 4 x 4 tiles, K = the 16 rows, computed transposed (h2^T dh3): wave 4 + mo takes output rows 16 mo .. and
        // ends up with four consecutive input columns per lane and tile
        const int mo = wave - 4;
        rows_gemm_fixed_b<4>(S + S_H2, LDC, S + S_DH3 + mo * 16, LDC, 0, 1, 4, [&](int nk, const f32x4 &acc) {
            pstore4(out, out_rsrc, O_W3 + (mo * 16 + i) * H + nk * 16 + 4 * g, acc, wt, keep);
        });
    }
    for (int e = tid; e < NA * H + NA + H; e += THREADS) {   // dW4, db4, db3
        float v = 0.f;
        if (e < NA * H) {
            const int a = e >> 6, kq = e & 63;
            for (int r = 0; r < ROWS; ++r)
                if (s_act[r >> 3] == a) v = fmaf(S[S_G + r], S[S_H3 + r * LDC + kq], v);
            pstore1(out + O_W4 + e, v, wt);
        } else if (e < NA * H + NA) {
            const int a = e - NA * H;
            for (int r = 0; r < ROWS; ++r)
                if (s_act[r >> 3] == a) v += S[S_G + r];
            pstore1(out + O_B4 + a, v, wt);
        } else {
            const int kq = e - NA * H - NA;
            for (int r = 0; r < ROWS; ++r) v += S[S_DH3 + r * LDC + kq];
            pstore1(out + O_B3 + kq, v, wt);
        }
    }
    __syncthreads();
    PH(10);  /* dh2, dW3, dW4 */
    {   // dx = dh2 W2 : 13 column tiles, first on every wave (the chain continues through them) ...
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = mma_a_lds<4>(S + S_DH2, LDC, bw.w2ta, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) S[S_DX + (4 * g + r) * LDF + wave * 16 + i] = acc[r];
        if (wave + 8 < NT1) {
            f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
            acc2 = mma_a_lds<4>(S + S_DH2, LDC, bw.w2tb, acc2);
#pragma unroll
            for (int r = 0; r < 4; ++r) S[S_DX + (4 * g + r) * LDF + (wave + 8) * 16 + i] = acc2[r];
        }
    }
    {   // ... then dW2 = dh2^T x : 4 x 13 tiles, computed transposed (x^T dh2; the dh2 tile 16 (w & 3) .. shared by the wave's 6-7 tiles):
        // acc[r] = dW2[16 mo + i][16 nk + 4 g + r] -> one 16-byte store per lane and tile
        const int mo = wave & 3;
        rows_gemm_fixed_b<7>(S + S_X, LDF, S + S_DH2 + mo * 16, LDC, wave >> 2, 2, NT1, [&](int nk, const f32x4 &acc) {
            pstore4(out, out_rsrc, O_W2 + (mo * 16 + i) * F + nk * 16 + 4 * g, acc, wt, keep);
        });
    }
    if (tid < H) {
        float v = 0.f;
        for (int r = 0; r < ROWS; ++r) v += S[S_DH2 + r * LDC + tid];
        pstore1(out + O_B2 + tid, v, wt);
    }
    __syncthreads();
    PH(11);  /* dx, dW2 */
    // Hadamard product: d(features) = sum over the sample's 8 rows of dx * h1;  d(pre-h1) = dx * features * [h1 > 0]
    for (int t = tid; t < BE * F; t += THREADS) {
        const int be = t / F, o = t - be * F;
        const float f = S[S_FEAT + t];
        float df = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int r = be * NQ + q;
            const float d = S[S_DX + r * LDF + o], h = S[S_H1 + r * LDF + o];
            df = fmaf(d, h, df);
            S[S_DX + r * LDF + o] = h > 0.f ? d * f : 0.f;
        }
        S[S_DF + t] = df;
    }
    __syncthreads();
    PH(12);  /* Hadamard */
    {   // dW1 = dh1^T cos : 13 x 4 tiles, computed transposed (cos^T dh1, the cos tile 16 (w & 3) .. shared by the wave's 6-7 tiles):
        // acc[r] = dW1[16 mo + i][16 nk + 4 g + r] -> one 16-byte store per lane and tile
        const int nk = wave & 3;
        rows_gemm_fixed_a<7>(S + S_C + nk * 16, LDC, S + S_DX, LDF, wave >> 2, 2, NT1, [&](int mo, const f32x4 &acc) {
            pstore4(out, out_rsrc, O_W1 + (mo * 16 + i) * NC + nk * 16 + 4 * g, acc, wt, keep);
        });
    }
    if (tid < F) {
        float v = 0.f;
        for (int r = 0; r < ROWS; ++r) v += S[S_DX + r * LDF + tid];
        pstore1(out + O_B1 + tid, v, wt);
    } else if (tid >= 256 && tid < 256 + F) {
        // encoders: dW = df^T obs, db = sum df
        const int o = tid - 256;
        const float d0 = S[S_DF + o], d1 = S[S_DF + F + o];
        const float *x0 = S + S_OBS, *x1 = S + S_OBS + 28;
        if (o < 16) {
            for (int kq = 0; kq < 2; ++kq) pstore1(out + O_VW + o * 2 + kq, fmaf(d1, x1[kq], d0 * x0[kq]), wt);
            pstore1(out + O_VB + o, d0 + d1, wt);
        } else if (o < 32) {
            for (int kq = 0; kq < 2; ++kq) pstore1(out + O_GW + (o - 16) * 2 + kq, fmaf(d1, x1[2 + kq], d0 * x0[2 + kq]), wt);
            pstore1(out + O_GB + o - 16, d0 + d1, wt);
        } else {
            pstore1(out + O_SB + o - 32, d0 + d1, wt);
        }
    }
    {   // sensor encoder dW [176 x 22] = 968 contiguous 16-byte pieces, one or two per thread (round 4: was 22 four-byte stores per lane at an
        // 88-byte stride -- 22 partial lines per lane, which write-through stores send to memory one by one); element (o, k) as before
        const float *x0 = S + S_OBS, *x1 = S + S_OBS + 28;
        for (int q = tid; q < 176 * 22 / 4; q += THREADS) {
            f32x4 v;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int e = 4 * q + c, o = 32 + e / 22, kq = e % 22;
                v[c] = fmaf(S[S_DF + F + o], x1[4 + kq], S[S_DF + o] * x0[4 + kq]);
            }
            pstore4(out, out_rsrc, O_SW + 4 * q, v, wt, keep);
        }
    }
    if (tid < P_PAD - P_TOTAL) pstore1(out + P_TOTAL + tid, 0.f, wt);   // row padding: read (as zeros) by the reduction's 16-byte loads
    PH(13);  /* dW1, encoder gradients issued */
    if (!two_roles && bid == 0) write_batch_copies(ba, base, batch);
    if (FUSED) {      // this workgroup's row (and loss partial) is final
        // Its stores are acknowledged -- by memory if they were write-through ones, by this XCD's L2 otherwise -- once vmcnt is 0; nothing of a
        // written-through row sits dirty in an L2: no __threadfence() (= an L2 write-back per workgroup, which made the first one-launch form 2.5 x slower)
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        PH(17);
#ifdef MN_TRAIN_PHASES
        if (tid_now() == 0) g_wgt[blockIdx.x][2] = wall_clock64();
#endif
        if (tid == 0) {
            if (wellplaced) *reinterpret_cast<volatile uint32_t *>(ws + ws_lflag(n_part) + 64 * (part & 7) + (part >> 3)) = tag;      // for this XCD's L2
            __hip_atomic_store((gu64 *)(ws + ws_done(n_part)) + part, ((uint64_t)tag << 32) | (wellplaced ? 0u : 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        group_reduce(ws, n_part, part, tag, tid);      // ... and this workgroup's share of its XCD group's row sum (self-tagged: nothing to wait for behind it)
        PH(18);
    }
#ifdef MN_TRAIN_PHASES
    __builtin_amdgcn_s_waitcnt(0);
    if (tid_now() == 0) g_wgt[blockIdx.x][1] = wall_clock64();
#endif
    }      // local workgroup
    }      // forward / backward of step k
    if (!FUSED) break;
    if ((is_target || is_extra) && k >= 1) {
        // ---- reduction + clip + Adam of step k - 1
        const int s = k - 1;
        const StepCtx sc = {epoch0 + (uint64_t)s, step0 + s, rs0, rs1 + (uint64_t)s, true, true};
        reduce_adam_body<2>(pb, n_phys, tail.n_virtual, ws, n_part, tail.grad, tail.loss_out + s, tail.rng_state, ba, tail.prefetch_next, tail.params, tail.m, tail.v,
                            tail.step, tail.lr, tail.b1, tail.b2, tail.eps, tail.max_norm, sc, XCHG ? tail.xa : nullptr, XCHG ? tail.xa_scale : 1.0f);
    }
    }      // k
