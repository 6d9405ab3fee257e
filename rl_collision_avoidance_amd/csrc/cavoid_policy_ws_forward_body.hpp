// cavoid_policy_ws_forward_body.hpp -- the body of policy_ws_forward_kernel<TRAIN> and policy_regression_ws_forward_kernel
// (cavoid_policy_ws.hpp includes it inside each; not a header of its own: no include guard, no namespace).  In scope: TRAIN, LOSS
// (kLossA3C / kLossRegression, read only where TRAIN) and the kernel argument `const PolicyWsArgs wa`.
    constexpr int RT = 4, kRows = 64;
    const PolicyArgs &p = wa.a;
    // LDS: rows [kRows][kPolStride], the packed biases, 8 ints, the tile's row list.  While the slots run, a row is
    //   cols 0..63 f_i (filter outputs of the current slot) | 80 raw num_other | 84..87 host | 88+8i..94+8i xn_i, 95+8i is_on_i
    extern __shared__ __attribute__((aligned(16))) float act[];
    float *lds_bias = act + kRows * kPolStride;
    int *ticket_slot = reinterpret_cast<int *>(lds_bias + kBiasFloats);
    int &ticket = ticket_slot[4];
    int *tile_row = ticket_slot + 8;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t row0 = (int64_t)blockIdx.x * kRows;
    const int64_t n_rows = (!TRAIN && p.row_count) ? (int64_t)*p.row_count : p.rows;
    const int rows_here = n_rows - row0 < kRows ? (int)(n_rows - row0 > 0 ? n_rows - row0 : 0) : kRows;
    const int M = p.max_other;
    const int step = (!TRAIN && p.actions_out) ? *p.step_counter : 0;
    if (!TRAIN && p.row_index && rows_here == 0) {
        if (p.actions_out) policy_finish(p, step, tid);
        return;
    }
    const WsLayout L = ws_layout(M);
    const int w1 = kPolHost + kPolHidden * M;              // layer1's input width (TRAIN: the row stride of l1_in)

    // ---- input tile: gather + normalise into the padded layout, is_on_i from the raw count ----------------------------
    if (!TRAIN && p.row_index) {
        if (tid < kRows) tile_row[tid] = tid < rows_here ? p.row_index[row0 + tid] : 0;
        __syncthreads();
    }
    const bool listed = !TRAIN && p.row_index != nullptr;
    {
        const float *src = listed ? p.x : p.x + row0 * p.stride;
        const int wpad = 16 + 8 * M + 8;                   // [num,0,0,0, host(4), M x (xn_i(7), is_on_i), 16 zeros]
        const float inv_wpad = 1.0f / (float)wpad;
        const int total = kRows * wpad;
        constexpr int U = 3 * RT;
        float bias_v[(kBiasFloats + 255) / 256];
#pragma unroll
        for (int u = 0; u < (kBiasFloats + 255) / 256; ++u) bias_v[u] = tid + 256 * u < kBiasFloats ? p.bias[tid + 256 * u] : 0.0f;
        if (tid == 0) {                                    // the CU arrival parity of policy_forward_kernel (static priority)
            const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
            const uint32_t key = ((xcc & 15u) << 8) | ((hw >> 8) & 0xFFu);
            ticket = (int)atomicAdd(p.cu_tickets + key, 1u);
        }
        for (int e0 = 0; e0 < total; e0 += 256 * U) {
            float v[U], av[U], sd[U], thr[U];
            int dst[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = e0 + u * 256 + tid;
                const int r = policy_div(e, wpad, inv_wpad), c = e - r * wpad;
                int sc = -1;                               // source column (-1: padding)
                float th = 0.0f;                           // > 0: is_on of slot th - 1 (source: the raw count)
                if (c == 0) sc = 0;
                else if (c >= 4 && c < 8) sc = c - 3;
                else if (c >= 8 && c < 8 + 8 * M) {
                    if ((c & 7) != 7) sc = 1 + kPolHost + kPolOther * ((c - 8) >> 3) + (c & 7);
                    else { sc = 0; th = (float)(((c - 8) >> 3) + 1); }
                }
                const bool in = e < total && sc >= 0 && r < rows_here;
                dst[u] = e < total ? r * kPolStride + kPolXCol + c : -1;
                v[u] = in ? src[(int64_t)(listed ? tile_row[r] : r) * p.stride + sc] : 0.0f;
                const bool norm = in && sc > 0 && p.avg != nullptr;
                av[u] = norm ? p.avg[sc] : 0.0f;
                sd[u] = norm ? p.std[sc] : 1.0f;
                thr[u] = th;
            }
            if (e0 == 0) {
#pragma unroll
                for (int u = 0; u < (kBiasFloats + 255) / 256; ++u)
                    if (tid + 256 * u < kBiasFloats) lds_bias[tid + 256 * u] = bias_v[u];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (dst[u] < 0) continue;
                act[dst[u]] = thr[u] > 0.0f ? (v[u] >= thr[u] ? 1.0f : 0.0f) : (v[u] - av[u]) / sd[u];
            }
        }
    }
    __syncthreads();
    if (ticket & 1) __builtin_amdgcn_s_setprio(1);
    if (TRAIN) {                                           // the host columns of layer1's input rows, and every slot's filter input
        for (int e = tid; e < kRows * kPolHost; e += 256) {
            const int r = e >> 2, k = e & 3;
            p.l1_in[(row0 + r) * w1 + k] = act[r * kPolStride + kPolXCol + 4 + k];
        }
        for (int e = tid; e < M * kRows * kWsFilterIn; e += 256) {
            const int i = e / (kRows * kWsFilterIn), r = (e >> 3) & (kRows - 1), k = e & 7;
            wa.f_in[((int64_t)i * p.rows64 + row0 + r) * kWsFilterIn + k] = act[r * kPolStride + kPolXCol + 8 + 8 * i + k];
        }
    }

    // ---- the slots: filter, then the slot's 4 K chunks of layer1 into the persistent accumulators -----------------------
    f32x4 acc[RT][4];
    policy_init_acc(lds_bias + kBiasL1, 4 * wave, lane, acc);
    const f32x4 fw = p.frags[L.filter + 64 * wave + lane];  // filter weights of this wavefront's 16 units (one K chunk)
    const float fb = lds_bias[kBiasOther + 16 * wave + (lane & 15)];
    const float *arow = act + (lane & 15) * kPolStride + 4 * (lane >> 4);
    float *frow = act + (4 * (lane >> 4)) * kPolStride + 16 * wave + (lane & 15);
    PolicyFrag<RT, 4> f0;
    for (int i = 0; i < M; ++i) {
        const f32x4 *l1 = p.frags + L.l1 + (int64_t)4 * i * kFragPerChunk;
        policy_load_b(f0, l1, 4 * wave, lane, 0);          // in flight across the filter and the barriers
        f32x4 fa[RT], facc[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            fa[rt] = *reinterpret_cast<const f32x4 *>(arow + 16 * rt * kPolStride + kPolXCol + 8 + 8 * i);
            facc[rt] = f32x4{fb, fb, fb, fb};
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) facc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[rt][s], fw[s], facc[rt], 0, 0, 0);
        __syncthreads();                                   // every wavefront has read f_{i-1}
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z = fmaxf(facc[rt][r], 0.0f);
                frow[(16 * rt + r) * kPolStride] = z;
                if (TRAIN) p.l1_in[(row0 + 16 * rt + 4 * (lane >> 4) + r) * w1 + kPolHost + kPolHidden * i + 16 * wave + (lane & 15)] = z;
            }
        __syncthreads();                                   // f_i is in place
        // the last slot also takes the host chunk (chunk 4 reads the host columns, as layer1 of the LSTM kernel does)
        policy_gemm(act, l1, 0, i + 1 < M ? 4 : 5, kPolXCol + 4, 4 * wave, lane, f0, acc);
    }
    policy_load_b(f0, p.frags + L.l2, 4 * wave, lane, 0);
    __syncthreads();
    policy_store_relu(act, 4 * wave, lane, acc, TRAIN ? p.z1 + row0 * kPolWidth : nullptr);
    __syncthreads();
    // ---- layer2, fullyconnected1, heads: policy_forward_kernel's ------------------------------------------------------
    {
        f32x4 acc2[RT][4];
        policy_init_acc(lds_bias + kBiasL2, 4 * wave, lane, acc2);
        policy_gemm(act, p.frags + L.l2, 0, kChWide, 64, 4 * wave, lane, f0, acc2);
        policy_load_b(f0, p.frags + L.fc1, 4 * wave, lane, 0);
        __syncthreads();
        policy_store_relu(act, 4 * wave, lane, acc2, TRAIN ? p.z2 + row0 * kPolWidth : nullptr);
        __syncthreads();
    }
    f32x4 hb[kChHead];
    {
        f32x4 acc3[RT][4];
        policy_init_acc(lds_bias + kBiasFc1, 4 * wave, lane, acc3);
        policy_gemm(act, p.frags + L.fc1, 0, kChWide, 64, 4 * wave, lane, f0, acc3);
        __syncthreads();
        policy_store_relu(act, 4 * wave, lane, acc3, TRAIN ? p.z3 + row0 * kPolWidth : nullptr);
        __syncthreads();
#pragma unroll
        for (int ch = 0; ch < kChHead / 2; ++ch) hb[ch] = p.frags[L.head + lane + 64 * ch];
    }
    policy_ws_heads<TRAIN, LOSS>(p, act, lds_bias, p.frags + L.head, hb, tile_row, listed, row0, rows_here, step, wave, lane);
    if (!TRAIN && p.actions_out) policy_finish(p, step, tid);
