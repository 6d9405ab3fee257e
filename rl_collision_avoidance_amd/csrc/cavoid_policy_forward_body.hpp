// cavoid_policy_forward_body.hpp -- the body of policy_forward_kernel<RT, TRAIN> and policy_regression_forward_kernel<RT>
// (cavoid_policy.hpp includes it inside each; not a header of its own: no include guard, no namespace).  In scope: RT, TRAIN,
// LOSS (kLossA3C / kLossRegression, read only where TRAIN) and the kernel argument `const PolicyArgs p`.
    constexpr int kRows = 16 * RT;
    // LDS: activations [kRows][kPolStride], then the packed biases, then one int.  While the LSTM runs, a row is
    //   cols 0..63 h | 80 raw num_other | 84..87 host | 88+8t..94+8t x_t (t-th observed agent), zeros between
    extern __shared__ __attribute__((aligned(16))) float act[];
    float *lds_bias = act + kRows * kPolStride;
    int *wave_max = reinterpret_cast<int *>(lds_bias + kBiasFloats);
    int &ticket = wave_max[4];
    int *tile_row = wave_max + 8;                          // [kRows] global row of each tile row (identity without a row list)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t row0 = (int64_t)blockIdx.x * kRows;
    const int64_t n_rows = (!TRAIN && p.row_count) ? (int64_t)*p.row_count : p.rows;
    const int rows_here = n_rows - row0 < kRows ? (int)(n_rows - row0 > 0 ? n_rows - row0 : 0) : kRows;
    const int M = p.max_other;
    const int step = (!TRAIN && p.actions_out) ? *p.step_counter : 0;
    if (!TRAIN && p.row_index && rows_here == 0) {         // uniform over the workgroup: nothing listed for this tile
        if (p.actions_out) policy_finish(p, step, threadIdx.x);
        return;
    }
    POLICY_STAMP(0);
#ifdef CAVOID_TRACE
    const unsigned long long trace_c0 = clock64();
    if (tid == 0 && g_pol_trace)
        g_pol_trace[(size_t)blockIdx.x * 16 + 7] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
                                                  ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
#endif
    const f32x4 *w_lstm = p.frags + kOffLstm;
    PolicyFrag<RT, 4> f0;
    policy_load_b(f0, w_lstm, 4 * wave, lane, 4);          // first LSTM step: h == 0, only the input chunk contributes

    // ---- input tile: gather + normalise into the padded layout above ------------------------------------------
    // One trip to memory: every global load of the prologue (inputs, normalisation vectors, biases) is issued
    // before the first of them is consumed.
    if (!TRAIN && p.row_index) {                           // one extra (tiny) trip to memory: the tile's row list
        if (tid < kRows) tile_row[tid] = tid < rows_here ? p.row_index[row0 + tid] : 0;
        __syncthreads();
    }
    const bool listed = !TRAIN && p.row_index != nullptr;
    {
        const float *src = listed ? p.x : p.x + row0 * p.stride;
        const int wpad = 16 + 8 * M + 8;                   // padded row: [num,0,0,0, host(4), M x (x_t(7),0), 16 zeros]
        const float inv_wpad = 1.0f / (float)wpad;
        const int total = kRows * wpad;
        constexpr int U = 3 * RT;                          // M = 3: the whole tile in one pass
        int local_max = 0;
        float bias_v[(kBiasFloats + 255) / 256];
#pragma unroll
        for (int u = 0; u < (kBiasFloats + 255) / 256; ++u) bias_v[u] = tid + 256 * u < kBiasFloats ? p.bias[tid + 256 * u] : 0.0f;
        if (tid == 0) {
            // Two workgroups share a CU (one wavefront of each per SIMD).  Arrival parity on the CU decides a static
            // priority, so that the pair does not settle into lockstep (same phase at the same time, the matrix
            // pipe idle while both do their pointwise / barrier phases): without it CU pairs finish anywhere between
            // 85 and 131 us, with it every pair takes the same time.
            const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
            const uint32_t key = ((xcc & 15u) << 8) | ((hw >> 8) & 0xFFu);        // cu_id[11:8] sh_id[12] se_id[15:13]
            ticket = (int)atomicAdd(p.cu_tickets + key, 1u);
        }
        for (int e0 = 0; e0 < total; e0 += 256 * U) {
            float v[U], av[U], sd[U];
            int dst[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {                  // all the loads of the pass first
                const int e = e0 + u * 256 + tid;
                const int r = policy_div(e, wpad, inv_wpad), c = e - r * wpad;
                int sc = -1;                               // source column of this slot (-1: padding)
                if (c == 0) sc = 0;
                else if (c >= 4 && c < 8) sc = c - 3;
                else if (c >= 8 && c < 8 + 8 * M && (c & 7) != 7) sc = 1 + kPolHost + kPolOther * ((c - 8) >> 3) + (c & 7);
                const bool in = e < total && sc >= 0 && r < rows_here;
                dst[u] = e < total ? r * kPolStride + kPolXCol + c : -1;
                v[u] = in ? src[(int64_t)(listed ? tile_row[r] : r) * p.stride + sc] : 0.0f;
                const bool norm = in && sc > 0 && p.avg != nullptr;
                av[u] = norm ? p.avg[sc] : 0.0f;
                sd[u] = norm ? p.std[sc] : 1.0f;
                if (sc != 0) dst[u] |= dst[u] >= 0 ? 0x40000000 : 0;      // tag: not the length column
            }
            if (e0 == 0) {
                for (int e = tid; e < kRows * kPolHidden; e += 256) act[(e >> 6) * kPolStride + (e & 63)] = 0.0f;   // h = 0
#pragma unroll
                for (int u = 0; u < (kBiasFloats + 255) / 256; ++u)
                    if (tid + 256 * u < kBiasFloats) lds_bias[tid + 256 * u] = bias_v[u];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (dst[u] < 0) continue;
                if (!(dst[u] & 0x40000000)) {
                    int len = (int)v[u];
                    len = len < 0 ? 0 : (len > M ? M : len);
                    local_max = local_max > len ? local_max : len;
                }
                act[dst[u] & 0x3FFFFFFF] = (v[u] - av[u]) / sd[u];
            }
        }
        // tile-wide maximum without an initialising barrier: wavefront maxima into 4 LDS slots
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_xor(local_max, d, 64); local_max = o > local_max ? o : local_max; }
        if (lane == 0) wave_max[wave] = local_max;
    }
    __syncthreads();
    const int m01 = wave_max[0] > wave_max[1] ? wave_max[0] : wave_max[1], m23 = wave_max[2] > wave_max[3] ? wave_max[2] : wave_max[3];
    const int tile_max_len = m01 > m23 ? m01 : m23;
    const int steps = tile_max_len;                        // LSTM steps any row of this tile still needs
    if (ticket & 1) __builtin_amdgcn_s_setprio(1);
    POLICY_STAMP(5);

    // this lane's rows in the C layout and their sequence lengths
    float len_r[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) len_r[rt][r] = act[(16 * rt + 4 * (lane >> 4) + r) * kPolStride + kPolXCol];

    // ---- LSTM over the observed agents -------------------------------------------------------------------
    f32x4 cell[RT], hid[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) { cell[rt] = f32x4{0.f, 0.f, 0.f, 0.f}; hid[rt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int t = 0; t < steps; ++t) {
        if (TRAIN) {                                       // the step's input rows, for the LSTM weight gradient
            float *dst = p.h_in + ((int64_t)t * p.rows64 + row0) * 72;
            for (int e = tid; e < kRows * 72; e += 256) {
                const int r = e / 72, k = e - r * 72;
                dst[e] = k < kPolHidden ? act[r * kPolStride + k]
                                        : (k < kPolHidden + kPolOther ? act[r * kPolStride + kPolXCol + 8 + 8 * t + (k - kPolHidden)] : 0.0f);
            }
        }
        f32x4 acc[RT][4];
        policy_init_acc(lds_bias + kBiasLstm, 4 * wave, lane, acc);
        if (t == 1) POLICY_STAMP(8);
        policy_gemm(act, w_lstm, t == 0 ? 4 : 0, kChLstm, kPolXCol + 8 + 8 * t, 4 * wave, lane, f0, acc);
        if (t == 1) POLICY_STAMP(9);
        policy_load_b(f0, w_lstm, 4 * wave, lane, 0);      // the next step's first weight fragments
        __syncthreads();                                   // every wavefront has read h
        if (t == 1) POLICY_STAMP(10);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // dynamic_rnn: rows past their own length keep (c, h) -- selects, not branches
                const bool live = len_r[rt][r] > (float)t;
                const float gi = fast_sigmoid(acc[rt][0][r]), gj = fast_tanh(acc[rt][1][r]);
                const float gf = fast_sigmoid(acc[rt][2][r]), go = fast_sigmoid(acc[rt][3][r]);
                float keep = gf * cell[rt][r], add = gi * gj;
                if (TRAIN) asm volatile("" : "+v"(keep), "+v"(add));   // (no packed add with swapped halves: DESIGN.md 3.7 (d))
                const float c_new = keep + add;
                const float tc = fast_tanh(c_new);
                const float h_new = go * tc;
                if (TRAIN) {                               // lane-private 32-byte records: the backward pass reads them back as is
                    f32x4 *sv = reinterpret_cast<f32x4 *>(p.save) + ((((int64_t)blockIdx.x * M + t) * 16 + (rt * 4 + r)) * 256 + tid) * 2;
                    sv[0] = f32x4{gi, gj, gf, go};
                    sv[1] = f32x4{cell[rt][r], tc, 0.0f, 0.0f};
                }
                cell[rt][r] = live ? c_new : cell[rt][r];
                hid[rt][r] = live ? h_new : hid[rt][r];
                act[(16 * rt + 4 * (lane >> 4) + r) * kPolStride + 16 * wave + (lane & 15)] = hid[rt][r];
            }
        if (t == 1) POLICY_STAMP(11);
        __syncthreads();                                   // the new h is in place
        if (t == 1) POLICY_STAMP(12);
    }
    POLICY_STAMP(1);
    // ---- layer1 on [h | host] --------------------------------------------------------------------------------
    {
        if (TRAIN) {                                       // layer1's input rows [h | host | 0], for its weight gradient
            float *dst = p.l1_in + row0 * 72;
            for (int e = tid; e < kRows * 72; e += 256) {
                const int r = e / 72, k = e - r * 72;
                dst[e] = k < kPolHidden ? act[r * kPolStride + k]
                                        : (k < kPolHidden + kPolHost ? act[r * kPolStride + kPolXCol + 4 + (k - kPolHidden)] : 0.0f);
            }
        }
        f32x4 acc[RT][4];
        policy_load_b(f0, p.frags + kOffL1, 4 * wave, lane, 0);
        policy_init_acc(lds_bias + kBiasL1, 4 * wave, lane, acc);
        policy_gemm(act, p.frags + kOffL1, 0, kChL1, kPolXCol + 4, 4 * wave, lane, f0, acc);
        policy_load_b(f0, p.frags + kOffL2, 4 * wave, lane, 0);
        __syncthreads();
        policy_store_relu(act, 4 * wave, lane, acc, TRAIN ? p.z1 + row0 * kPolWidth : nullptr);
        __syncthreads();
    }
    POLICY_STAMP(2);
    // ---- layer2, fullyconnected1 -----------------------------------------------------------------------------
    {
        f32x4 acc[RT][4];
        policy_init_acc(lds_bias + kBiasL2, 4 * wave, lane, acc);
        policy_gemm(act, p.frags + kOffL2, 0, kChWide, 64, 4 * wave, lane, f0, acc);
        policy_load_b(f0, p.frags + kOffFc1, 4 * wave, lane, 0);
        __syncthreads();
        policy_store_relu(act, 4 * wave, lane, acc, TRAIN ? p.z2 + row0 * kPolWidth : nullptr);
        __syncthreads();
    }
    f32x4 hb[kChHead];                                     // the heads' weight fragments: in flight across the last layer's
    {                                                      // epilogue and barrier
        f32x4 acc[RT][4];
        policy_init_acc(lds_bias + kBiasFc1, 4 * wave, lane, acc);
        policy_gemm(act, p.frags + kOffFc1, 0, kChWide, 64, 4 * wave, lane, f0, acc);
        const f32x4 *brow = p.frags + kOffHead + lane;
        if (RT == 4 && !TRAIN) {                           // 2 wavefronts per SIMD: the registers are there
#pragma unroll
            for (int ch = 0; ch < kChHead; ++ch) hb[ch] = brow[64 * ch];
        }
        __syncthreads();
        policy_store_relu(act, 4 * wave, lane, acc, TRAIN ? p.z3 + row0 * kPolWidth : nullptr);
        __syncthreads();
        if (RT != 4 || TRAIN) {                            // tighter register budget: half now, half below
#pragma unroll
            for (int ch = 0; ch < kChHead / 2; ++ch) hb[ch] = brow[64 * ch];
        }
    }
    POLICY_STAMP(3);
    // ---- heads: wavefront w < RT does rows 16w..16w+15 x 16 columns (A logits, the value, padding) ------------
    if (wave < RT) {
        f32x4 acc[4];
        const float b = lds_bias[kBiasHead + (lane & 15)];
        acc[0] = f32x4{b, b, b, b};
        acc[1] = acc[2] = acc[3] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *arow = act + (16 * wave + (lane & 15)) * kPolStride + 4 * (lane >> 4);
#pragma unroll
        for (int g = 0; g < kChHead; g += 4) {
            if ((RT != 4 || TRAIN) && g == 0) {
#pragma unroll
                for (int ch = kChHead / 2; ch < kChHead; ++ch) hb[ch] = p.frags[kOffHead + lane + 64 * ch];
            }
            f32x4 ha[4];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) ha[ch] = *reinterpret_cast<const f32x4 *>(arow + 16 * (g + ch));
#pragma unroll
            for (int ch = 0; ch < 4; ++ch)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[ch][s], hb[g + ch][s], acc[s], 0, 0, 0);
        }
        const f32x4 logit = acc[0] + acc[1] + acc[2] + acc[3];
        const int col = lane & 15, A = p.num_actions;
        const float scale = 1.0f / (1.0f + p.min_policy * (float)A);
        float cost_p = 0.0f, cost_v = 0.0f, gsum = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float z = logit[r];
            float m = col < A ? z : -INFINITY;
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) m = fmaxf(m, __shfl_xor(m, d, 16));
            const float e = col < A ? expf(z - m) : 0.0f;
            float sum = e;
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) sum += __shfl_xor(sum, d, 16);
            const int trow = 16 * wave + 4 * (lane >> 4) + r;             // row of the tile
            const bool in_tile = TRAIN || trow < rows_here;
            const int64_t row = listed ? (in_tile ? (int64_t)tile_row[trow] : p.rows) : row0 + trow;     // global row
            const float sm = e / sum;                      // softmax
            const float pj = col < A ? (sm + p.min_policy) * scale : 0.0f;
            if (!TRAIN && row < p.rows) {
                if (col < A) p.p_out[row * A + col] = pj;
                else if (col == A) p.v_out[row] = z;
            }
            if (TRAIN && LOSS == kLossRegression) {
                const float g = policy_regression_head(p, row, col, A, z, m, e, sum, cost_p, cost_v);
                p.gh[(row0 + 16 * wave + 4 * (lane >> 4) + r) * 16 + col] = g;
                gsum += g;
            }
            if (TRAIN && LOSS == kLossA3C) {
                // A3C loss of NetworkVPCore.py:71-100 (sums over rows) and its gradient at the logits:
                //   cost_v = 0.5 (y - v)^2;  cost_p = -[ log(max(p_a, eps)) (y - v_detached) - beta sum_k log(max(p_k, eps)) p_k ]
                const bool valid = row < p.rows;
                const float y = valid ? p.y_r[row] : 0.0f;
                const int a = valid ? p.a_idx[row] : 0;
                const float v = __shfl(z, A, 16);
                const float sel = __shfl(pj, a, 16);
                const float lp = __logf(fmaxf(pj, p.log_eps));
                // d cost_p / d p'_k, then through p' = (softmax + MIN_POLICY) * scale and the softmax
                float dp = p.beta * (pj > p.log_eps ? lp + 1.0f : lp);
                if (col == a && sel > p.log_eps) dp -= (y - v) / sel;
                dp = col < A ? dp * scale : 0.0f;
                float dot = sm * dp;
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) dot += __shfl_xor(dot, d, 16);
                float g = col < A ? sm * (dp - dot) : (col == A ? v - y : 0.0f);
                if (!valid) g = 0.0f;
                p.gh[(row0 + 16 * wave + 4 * (lane >> 4) + r) * 16 + col] = g;
                gsum += g;
                float ent = col < A ? lp * pj : 0.0f;
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) ent += __shfl_xor(ent, d, 16);
                if (valid && col == 0) {
                    cost_p -= __logf(fmaxf(sel, p.log_eps)) * (y - v) - p.beta * ent;
                    cost_v += 0.5f * (y - v) * (y - v);
                }
            }
            if (!TRAIN && p.actions_out) {                 // wave-uniform
                int action;
                if (p.greedy) {                            // np.argmax: first index of the maximum
                    float best = pj;
#pragma unroll
                    for (int d = 1; d < 16; d <<= 1) best = fmaxf(best, __shfl_xor(best, d, 16));
                    int idx = (col < A && pj == best) ? col : 99;
#pragma unroll
                    for (int d = 1; d < 16; d <<= 1) { const int o = __shfl_xor(idx, d, 16); idx = o < idx ? o : idx; }
                    action = idx;
                } else {                                   // inverse CDF: #{c : cdf_c <= u * cdf_{A-1}}
                    float cdf = pj;
#pragma unroll
                    for (int d = 1; d < 16; d <<= 1) { const float t = __shfl_up(cdf, d, 16); if (col >= d) cdf += t; }
                    const float total = __shfl(cdf, A - 1, 16);
                    const uint32_t bits = policy_philox_x((uint32_t)row, (uint32_t)((uint64_t)row >> 32), (uint32_t)step, 0x504F4Cu,
                                                          p.seed_lo, p.seed_hi);
                    const float u = (float)(bits >> 8) * (1.0f / 16777216.0f);
                    int below = (col < A && cdf <= u * total) ? 1 : 0;
#pragma unroll
                    for (int d = 1; d < 16; d <<= 1) below += __shfl_xor(below, d, 16);
                    action = below < A - 1 ? below : A - 1;
                }
                if (row < p.rows && col == 0) p.actions_out[row] = action;
            }
        }
        if (TRAIN) {                                       // one atomic pair per wavefront
            cost_p += __shfl_xor(cost_p, 16, 64); cost_p += __shfl_xor(cost_p, 32, 64);
            cost_v += __shfl_xor(cost_v, 16, 64); cost_v += __shfl_xor(cost_v, 32, 64);
            if (lane == 0) { atomicAdd(p.loss, cost_p); atomicAdd(p.loss + 1, cost_v); }
            gsum += __shfl_xor(gsum, 16, 64); gsum += __shfl_xor(gsum, 32, 64);
            if (lane < 16) atomicAdd(p.db + kBiasHead + lane, gsum);
        }
    }
    POLICY_STAMP(4);
#ifdef CAVOID_TRACE
    if (tid == 0 && g_pol_trace) g_pol_trace[(size_t)blockIdx.x * 16 + 6] = clock64() - trace_c0;   // shader-clock cycles
#endif
    if (!TRAIN && p.actions_out) policy_finish(p, step, tid);
