// cavoid_policy_ws.hpp -- NetworkVP_rnn with MULTI_AGENT_ARCH 'weight_sharing' on the gfx950 matrix cores: the actors'
// predict_p_and_v + select_action as ONE kernel (policy_ws_forward_kernel<false>) and the trainer's pass as two
// (policy_ws_forward_kernel<true>: forward + A3C loss + gradient at the heads; policy_ws_backward_kernel: the row-local backward).
// The supervised start's pass is the same pair with the other loss head (policy_regression_ws_forward_kernel: cost_regression).
//
// What it computes (citations: ga3c/GA3C/NetworkVP_rnn.py in the reference:50-61,69-92,103-105, NetworkVPCore.py:66-75):
//   xn = (x - avg) / std (optional);  is_on_i = x[:,0] >= i + 1 on the RAW count
//   f_i = relu([xn_i (7) | is_on_i] . other_kernel[8, 64] + other_bias)     for EVERY slot i < M (also past the row's count)
//   layer1 = relu([host(4) | f_0 .. f_{M-1}] . layer1_kernel[4 + 64M, 256] + b), then layer2, fullyconnected1, heads and
//   softmax + MIN_POLICY exactly as policy_forward_kernel (cavoid_policy.hpp) does them.
//
// Layout: the float32-MFMA machinery of cavoid_policy.hpp (v_mfma_f32_16x16x4_f32: exact float32 products), one 64-row tile per
// workgroup of 4 wavefronts, the same LDS rows [64][260] (71 008 B, 2 workgroups per CU).  The input row is parked as the LSTM
// kernel parks it (count and host at columns 80..87, slot i at 88 + 8i) with is_on_i in the slot's 8th column, zero there.  The
// slots are a loop: wavefront w computes filter units 16w..16w+15 of slot i for the tile's 64 rows (one K chunk, 16 MFMAs), the
// 64 outputs go to LDS columns 0..63 (the LSTM's h columns), and the slot's 4 K chunks of layer1 accumulate into the persistent
// layer1 accumulators.  Nothing in LDS grows with M: M <= 19 is bounded by the parked row (80 + 16 + 8M + 8 <= 260, kPolMaxOthers)
// and the weight pack stays L2-resident (layer1 is 16 KB per K chunk, (4M + 1) chunks: 1.25 MB at M = 19).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cavoid_policy.hpp"

namespace cavoid {

constexpr int kWsMaxOthers = kPolMaxOthers;   // mirrored by ga3c/policy_kernel.py MAX_OTHERS_WS (tests/test_policy_ws_host.py)
constexpr int kWsOthersRange = 64;        // what cavoid_policy_create_ws tells apart from a bad argument (the env's own limit)
constexpr int kWsFilterIn = kPolOther + 1;    // 7 features + is_on
constexpr int kBiasOther = kBiasLstm;         // other_bias takes the first 64 of the LSTM's 256 packed bias slots

// Fragment offsets (in float4 = one lane's 4 k-values) of the weight-sharing pack.  Forward: filter (1 chunk of K = 16, rows 8..15
// zero, 4 column tiles), layer1 (4M + 1 chunks: slot i = chunks 4i..4i+3, the host last), layer2, fc1 (16 chunks), heads (16 chunks x
// 1 column tile).  Transposed, for the trainer: heads^T (1 chunk), fc1^T, layer2^T (16 chunks), layer1^T per slot (K = 256, N = 64).
struct WsLayout {
    int64_t filter, l1, l2, fc1, head, fwd_end, thead, tfc1, tl2, tl1, end;
};
__host__ __device__ constexpr WsLayout ws_layout(int M) {
    const int64_t l1 = kFragPerChunkNarrow, l2 = l1 + (4 * (int64_t)M + 1) * kFragPerChunk, fc1 = l2 + kChWide * kFragPerChunk;
    const int64_t head = fc1 + kChWide * kFragPerChunk, fwd_end = head + kChHead * 64;
    const int64_t tfc1 = fwd_end + kFragPerChunk, tl2 = tfc1 + kChWide * kFragPerChunk, tl1 = tl2 + kChWide * kFragPerChunk;
    return WsLayout{0, l1, l2, fc1, head, fwd_end, fwd_end, tfc1, tl2, tl1, tl1 + (int64_t)M * kChWide * kFragPerChunkNarrow};
}

struct PolicyWsWeights {               // device pointers, TensorFlow layout ([in, out] kernels)
    const float *other_kernel, *other_bias;    // [8, 64]: 7 inputs then is_on
    const float *layer1_kernel, *layer1_bias;  // [4 + 64M, 256]: 4 host rows, then slot-major
    const float *layer2_kernel, *layer2_bias, *fc1_kernel, *fc1_bias, *p_kernel, *p_bias, *v_kernel, *v_bias;
    int num_actions, max_other;
};

// element [k][col] of packed layer `layer` (0 filter, 1 layer1 with k over all 4M + 1 chunks, 2 layer2, 3 fc1, 4 heads; 5 heads^T,
// 6 fc1^T, 7 layer2^T, 8 layer1^T with k = 256 * slot + output unit)
__device__ __forceinline__ float policy_ws_weight(const PolicyWsWeights &w, int layer, int k, int col) {
    const int M = w.max_other;
    switch (layer) {
    case 0: return k < kWsFilterIn ? w.other_kernel[k * kPolHidden + col] : 0.0f;
    case 1:
        if (k < kPolHidden * M) return w.layer1_kernel[(int64_t)(kPolHost + k) * kPolWidth + col];
        return k - kPolHidden * M < kPolHost ? w.layer1_kernel[(int64_t)(k - kPolHidden * M) * kPolWidth + col] : 0.0f;
    case 2: return w.layer2_kernel[(int64_t)k * kPolWidth + col];
    case 3: return w.fc1_kernel[(int64_t)k * kPolWidth + col];
    case 4:
        if (col < w.num_actions) return w.p_kernel[(int64_t)k * w.num_actions + col];
        return col == w.num_actions ? w.v_kernel[k] : 0.0f;
    case 5:
        if (k < w.num_actions) return w.p_kernel[(int64_t)col * w.num_actions + k];
        return k == w.num_actions ? w.v_kernel[col] : 0.0f;
    case 6: return w.fc1_kernel[(int64_t)col * kPolWidth + k];
    case 7: return w.layer2_kernel[(int64_t)col * kPolWidth + k];
    default: {
        const int slot = k >> 8, unit = k & 255;
        return w.layer1_kernel[(int64_t)(kPolHost + kPolHidden * slot + col) * kPolWidth + unit];
    }
    }
}

#ifdef CAVOID_POLICY_WS_KERNELS  /* non-template kernel: compiled by cavoid_policy_ws.hip only */
// frags[f] for f < n_frags (ws_layout(M).fwd_end, or .end with the transposed copies); bias[1040] in packed order:
// other_bias 64 | 0 | layer1 256 | layer2 256 | fc1 256 | heads 16
__global__ void __launch_bounds__(256) policy_ws_pack_kernel(const PolicyWsWeights w, f32x4 *frags, float *bias, int64_t n_frags) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const WsLayout L = ws_layout(w.max_other);
    if (f < n_frags) {
        int layer, chunk, ct, lane;
        if (f < L.l1 || f >= L.tl1) {                      // narrow layers: 4 column tiles per chunk
            const int64_t r = f - (f < L.l1 ? L.filter : L.tl1);
            layer = f < L.l1 ? 0 : 8;
            chunk = (int)(r / kFragPerChunkNarrow); ct = (int)((r >> 6) & 3); lane = (int)(r & 63);
        } else if (f >= L.head && f < L.fwd_end) {
            const int64_t r = f - L.head;
            layer = 4; chunk = (int)(r >> 6); ct = 0; lane = (int)(r & 63);
        } else {
            const int64_t base = f >= L.tl2 ? L.tl2 : f >= L.tfc1 ? L.tfc1 : f >= L.thead ? L.thead : f >= L.fc1 ? L.fc1 : f >= L.l2 ? L.l2 : L.l1;
            layer = f >= L.tl2 ? 7 : f >= L.tfc1 ? 6 : f >= L.thead ? 5 : f >= L.fc1 ? 3 : f >= L.l2 ? 2 : 1;
            const int64_t r = f - base;
            chunk = (int)(r / kFragPerChunk); ct = (int)((r >> 6) & 15); lane = (int)(r & 63);
        }
        const int k0 = 16 * chunk + 4 * (lane >> 4), col = 16 * ct + (lane & 15);
        f32x4 v;
        v.x = policy_ws_weight(w, layer, k0 + 0, col); v.y = policy_ws_weight(w, layer, k0 + 1, col);
        v.z = policy_ws_weight(w, layer, k0 + 2, col); v.w = policy_ws_weight(w, layer, k0 + 3, col);
        frags[f] = v;
    }
    if (f < kBiasFloats) {
        const int i = (int)f;
        float b;
        if (i < kBiasL1) b = i < kPolHidden ? w.other_bias[i] : 0.0f;
        else if (i < kBiasL2) b = w.layer1_bias[i - kBiasL1];
        else if (i < kBiasFc1) b = w.layer2_bias[i - kBiasL2];
        else if (i < kBiasHead) b = w.fc1_bias[i - kBiasFc1];
        else {
            const int c = i - kBiasHead;
            b = c < w.num_actions ? w.p_bias[c] : (c == w.num_actions ? w.v_bias[0] : 0.0f);
        }
        bias[i] = b;
    }
}
#endif

// The policy_forward_kernel arguments, plus the TRAIN pass's weight-sharing buffers.  In the TRAIN instantiation a.l1_in is
// [rows64, 4 + 64M] in the checkpoint's row order (host, then slot-major: d layer1 = l1_in^T g1 needs no re-indexing);
// a.h_in and a.save are unused.
struct PolicyWsArgs {
    PolicyArgs a;
    float *f_in;                       // [M, rows64, 8] filter inputs [xn_i | is_on_i] (TRAIN only)
};

// The forward pass of one 64-row tile: policy_ws_forward_kernel<TRAIN> (LOSS = kLossA3C) and policy_regression_ws_forward_kernel
// (TRAIN with LOSS = kLossRegression) are thin kernels over it.  Ring (PolNoRing / PolRing<R>, cavoid_policy.hpp): whether the input
// slots hold the whole row (M <= kWsMaxOthers) or are a ring of R slots refilled while the slot loop runs (the kernels and the
// protocol of cavoid_policy_wsring.hpp).
//
// FUSED = true: the pass as ONE PHASE of a kernel that goes on (actor_ws_kernel, cavoid_actor_ws.hpp; with the ring crowd_ws_rollout_kernel,
// cavoid_crowd_actor_ws.hpp: the ring's refills go through the caller's row list like the staging) instead of a whole launch.  The
// caller hands over what the launch forms derive from the grid and the device-side counters: the thread id (`tid_in`; its step loop
// re-materialises it), the tile's rows as a list it has written to the LDS row list (ws_tile_row(): `rows_in` GLOBAL rows, the row-list
// form's gather from p.x and its scatter of the outputs) and the step that keys the action draw (`step_in`).  The CU ticket is the
// caller's (taken once per launch, at ws_ticket_slot()[4]), there is no policy_finish and no p.p_out.  Every statement that computes a
// row's outputs is the launch forms': the results are theirs bit for bit.
template <bool TRAIN, int LOSS, class Ring = PolNoRing, bool FUSED = false>
__device__ __forceinline__ void policy_ws_forward_tile(const PolicyWsArgs &wa, int tid_in = 0, int rows_in = 0, int step_in = 0) {
    static_assert(!FUSED || !TRAIN, "the fused phase is the actors' pass (whole-row, or with the ring: crowd_ws_rollout_kernel)");
    constexpr int RT = 4, kRows = 64;
    const PolicyArgs &p = wa.a;
    // LDS: rows [kRows][kPolStride], the packed biases, 8 ints, the tile's row list.  While the slots run, a row is
    //   cols 0..63 f_i (filter outputs of the current slot) | 80 raw num_other | 84..87 host | 88+8i..94+8i xn_i, 95+8i is_on_i
    //   (with a ring: 88+8s.. the slot parked in ring slot s)
    extern __shared__ __attribute__((aligned(16))) float act[];
    float *lds_bias = act + kRows * kPolStride;
    int *ticket_slot = reinterpret_cast<int *>(lds_bias + kBiasFloats);
    int &ticket = ticket_slot[4];
    int *tile_row = ticket_slot + 8;
    const int tid = FUSED ? tid_in : (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t row0 = FUSED ? 0 : (int64_t)blockIdx.x * kRows;
    int rows_here_v, step_v;
    if constexpr (FUSED) {
        rows_here_v = rows_in; step_v = step_in;
    } else {
        const int64_t n_rows = (!TRAIN && p.row_count) ? (int64_t)*p.row_count : p.rows;
        rows_here_v = n_rows - row0 < kRows ? (int)(n_rows - row0 > 0 ? n_rows - row0 : 0) : kRows;
        step_v = (!TRAIN && p.actions_out) ? *p.step_counter : 0;
    }
    const int rows_here = rows_here_v, step = step_v;
    const int M = p.max_other;
    if (!FUSED && !TRAIN && p.row_index && rows_here == 0) {
        if (p.actions_out) policy_finish(p, step, tid);
        return;
    }
    const WsLayout L = ws_layout(M);
    const int w1 = kPolHost + kPolHidden * M;              // layer1's input width (TRAIN: the row stride of l1_in)

    // ---- input tile: gather + normalise into the padded layout, is_on_i from the raw count ----------------------------
    if (!FUSED && !TRAIN && p.row_index) {
        if (tid < kRows) tile_row[tid] = tid < rows_here ? p.row_index[row0 + tid] : 0;
        __syncthreads();
    }
    const bool listed = FUSED || (!TRAIN && p.row_index != nullptr);      // (FUSED: the caller's list, behind a barrier of its own)
    const float *src = listed ? p.x : p.x + row0 * p.stride;
    int staged = M;                                        // slots the staging parks (a ring: the first R)
    if constexpr (Ring::on) staged = M < Ring::R ? M : Ring::R;
    {
        const int wpad = 16 + 8 * staged + 8;              // [num,0,0,0, host(4), staged x (xn_i(7), is_on_i), 16 zeros]
        const float inv_wpad = 1.0f / (float)wpad;
        const int total = kRows * wpad;
        constexpr int U = 3 * RT;
        float bias_v[(kBiasFloats + 255) / 256];
#pragma unroll
        for (int u = 0; u < (kBiasFloats + 255) / 256; ++u) bias_v[u] = tid + 256 * u < kBiasFloats ? p.bias[tid + 256 * u] : 0.0f;
        if (!FUSED && tid == 0) ticket = policy_cu_ticket(p.cu_tickets);
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
                else if (c >= 8 && c < 8 + 8 * staged) {
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
    if (!FUSED && (ticket & 1)) __builtin_amdgcn_s_setprio(1);
    if (TRAIN) {                                           // the host columns of layer1's input rows, and every slot's filter input
        for (int e = tid; e < kRows * kPolHost; e += 256) {
            const int r = e >> 2, k = e & 3;
            p.l1_in[(row0 + r) * w1 + k] = act[r * kPolStride + kPolXCol + 4 + k];
        }
        if constexpr (!Ring::on) {                         // (a ring: per iteration, from the ring slot)
            for (int e = tid; e < M * kRows * kWsFilterIn; e += 256) {
                const int i = e / (kRows * kWsFilterIn), r = (e >> 3) & (kRows - 1), k = e & 7;
                wa.f_in[((int64_t)i * p.rows64 + row0 + r) * kWsFilterIn + k] = act[r * kPolStride + kPolXCol + 8 + 8 * i + k];
            }
        }
    }

    // the ring's element e = tid + 256 u of one slot's 64 x 8 values -- tile row e / 8, column e % 8 (7: is_on).  ring_src: the row's
    // first float in global memory, -1 for a tile row at or past rows_here (zeros); ring_cnt: the row's raw count
    [[maybe_unused]] int ring_lds[2], ring_k[2];
    [[maybe_unused]] int64_t ring_src[2];
    [[maybe_unused]] float ring_cnt[2];
    if constexpr (Ring::on) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = tid + 256 * u, r = e >> 3;
            ring_k[u] = e & 7;
            ring_lds[u] = r * kPolStride + kPolXCol + 8 + ring_k[u];
            ring_src[u] = r < rows_here ? (int64_t)(listed ? tile_row[r] : r) * p.stride : -1;
            ring_cnt[u] = act[r * kPolStride + kPolXCol];
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
    [[maybe_unused]] int slot = 0;                         // i % R
    for (int i = 0; i < M; ++i) {
        const f32x4 *l1 = p.frags + L.l1 + (int64_t)4 * i * kFragPerChunk;
        policy_load_b(f0, l1, 4 * wave, lane, 0);          // in flight across the filter and the barriers
        // slot i + R into registers (uniform): in flight across the filter MFMAs and the first barrier
        [[maybe_unused]] bool refill = false;
        [[maybe_unused]] float rv[2], rav[2], rsd[2];
        if constexpr (Ring::on) {
            refill = i + Ring::R < M;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int sc = 1 + kPolHost + kPolOther * (i + Ring::R) + ring_k[u];
                const bool in = refill && ring_src[u] >= 0 && ring_k[u] < kPolOther;
                rv[u] = in ? src[ring_src[u] + sc] : 0.0f;
                const bool norm = in && p.avg != nullptr;
                rav[u] = norm ? p.avg[sc] : 0.0f;
                rsd[u] = norm ? p.std[sc] : 1.0f;
            }
        }
        const int scol = kPolXCol + 8 + 8 * (Ring::on ? slot : i);     // the LDS slot that holds input slot i
        if constexpr (Ring::on) {
            if (TRAIN) {                                   // the slot's filter input rows, for the filter's weight gradient
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    wa.f_in[((int64_t)i * p.rows64 + row0 + ((tid + 256 * u) >> 3)) * kWsFilterIn + ring_k[u]] = act[ring_lds[u] + 8 * slot];
            }
        }
        f32x4 fa[RT], facc[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            fa[rt] = *reinterpret_cast<const f32x4 *>(arow + 16 * rt * kPolStride + scol);
            facc[rt] = f32x4{fb, fb, fb, fb};
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) facc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[rt][s], fw[s], facc[rt], 0, 0, 0);
        __syncthreads();                                   // every wavefront has read f_{i-1} (and ring slot i % R)
        if constexpr (Ring::on) {
            if (refill) {                                  // is_on from the raw count, as the staging takes it
                const float thr = (float)(i + Ring::R + 1);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const float on = ring_src[u] >= 0 && ring_cnt[u] >= thr ? 1.0f : 0.0f;
                    act[ring_lds[u] + 8 * slot] = ring_k[u] == kPolOther ? on : (rv[u] - rav[u]) / rsd[u];
                }
            }
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z = fmaxf(facc[rt][r], 0.0f);
                frow[(16 * rt + r) * kPolStride] = z;
                if (TRAIN) p.l1_in[(row0 + 16 * rt + 4 * (lane >> 4) + r) * w1 + kPolHost + kPolHidden * i + 16 * wave + (lane & 15)] = z;
            }
        __syncthreads();                                   // f_i (and the refilled slot) is in place
        // the last slot also takes the host chunk (chunk 4 reads the host columns, as layer1 of the LSTM kernel does)
        policy_gemm(act, l1, 0, i + 1 < M ? 4 : 5, kPolXCol + 4, 4 * wave, lane, f0, acc);
        if constexpr (Ring::on) slot = slot + 1 == Ring::R ? 0 : slot + 1;
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
    policy_heads<RT, TRAIN, LOSS, false, !FUSED>(p, act, lds_bias, p.frags + L.head, hb, tile_row, listed, row0, rows_here, step, wave, lane);
    if (!FUSED && !TRAIN && p.actions_out) policy_finish(p, step, tid);
}

// the tile's LDS words behind the activation rows and the packed biases (policy_lds_bytes(4)): 8 ints ([4]: the CU ticket) and the
// 64-entry row list -- for a caller of the FUSED form, which owns the ticket and writes the list
__device__ __forceinline__ int *ws_ticket_slot(float *act) { return reinterpret_cast<int *>(act + 64 * kPolStride + kBiasFloats); }
__device__ __forceinline__ int *ws_tile_row(float *act) { return ws_ticket_slot(act) + 8; }

template <bool TRAIN>
__global__ void __launch_bounds__(256, TRAIN ? 1 : 2) policy_ws_forward_kernel(const PolicyWsArgs wa) {
    policy_ws_forward_tile<TRAIN, kLossA3C>(wa);
}

#ifdef CAVOID_POLICY_WS_KERNELS  /* non-template kernels: compiled by cavoid_policy_ws.hip only */
// The supervised start's trainer pass (cavoid_policy_train_regression_ws): the TRAIN forward with the regression head.  It leaves
// what policy_ws_forward_kernel<true> leaves, so that policy_ws_backward_kernel runs behind it unchanged.
__global__ void __launch_bounds__(256, 1) policy_regression_ws_forward_kernel(const PolicyWsArgs wa) {
    policy_ws_forward_tile<true, kLossRegression>(wa);
}

// ---- backward (trainer) ---------------------------------------------------------------------------------
// heads^T, fullyconnected1^T, layer2^T exactly as policy_backward_kernel (masked gradients g3, g2, g1 and their column sums), then
// per slot d f_i = g1 . layer1[4 + 64i .. 4 + 64i + 63, :]^T (one column tile of 16 units per wavefront), masked by f_i > 0 (read
// back from l1_in) -> gf [M, rows64, 64], column sums into db[0..64) (other_bias).  The weight gradients are the caller's GEMMs:
// d layer1 = l1_in^T g1 and d other_kernel = f_in^T gf over all M * rows64 rows.
struct PolicyWsBackArgs {
    int64_t rows64;
    int max_other;
    const f32x4 *frags;
    const float *z1, *z2, *z3, *gh, *l1_in;
    float *g1, *g2, *g3;               // [rows64, 256]
    float *gf;                         // [M, rows64, 64]
    float *db;                         // [kBiasFloats] packed bias order (other_bias at 0..63)
};

// One workgroup per CU: at two, the slot loop's narrow GEMM pushes the register budget of 256 into 308 B/lane of scratch
// (332 registers at one).
__global__ void __launch_bounds__(256, 1) policy_ws_backward_kernel(const PolicyWsBackArgs p) {
    constexpr int RT = 4, kRows = 64;
    extern __shared__ __attribute__((aligned(16))) float act[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t row0 = (int64_t)blockIdx.x * kRows;
    const int M = p.max_other;
    const WsLayout L = ws_layout(M);
    const int w1 = kPolHost + kPolHidden * M;

    PolicyFrag<RT, 4> f0;
    policy_load_b(f0, p.frags + L.thead, 4 * wave, lane, 0);
    for (int e = tid; e < kRows * 16; e += 256) act[(e >> 4) * kPolStride + (e & 15)] = p.gh[row0 * 16 + e];
    __syncthreads();
    policy_backward_wide(act, p.frags + L.thead, p.frags + L.tfc1, p.frags + L.tl2, f0, p.z1, p.z2, p.z3, p.g1, p.g2, p.g3, p.db, row0, wave, lane);
    // ---- layer1^T per slot (g1 stays in LDS, read only): the filter outputs' gradient, masked by the filter's relu --------
    const int col = 16 * wave + (lane & 15);
    PolicyFrag<RT, 1> n0;
    for (int i = 0; i < M; ++i) {
        const f32x4 *tl1 = p.frags + L.tl1 + (int64_t)i * kChWide * kFragPerChunkNarrow;
        f32x4 acc1[RT][1];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc1[rt][0] = f32x4{0.f, 0.f, 0.f, 0.f};
        policy_load_b(n0, tl1, wave, lane, 0);
        policy_gemm(act, tl1, 0, kChWide, 64, wave, lane, n0, acc1);
        float bsum = 0.0f;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = row0 + 16 * rt + 4 * (lane >> 4) + r;
                const float f = p.l1_in[row * w1 + kPolHost + kPolHidden * i + col];
                const float g = f > 0.0f ? acc1[rt][0][r] : 0.0f;
                p.gf[((int64_t)i * p.rows64 + row) * kPolHidden + col] = g;
                bsum += g;
            }
        bsum += __shfl_xor(bsum, 16, 64);
        bsum += __shfl_xor(bsum, 32, 64);
        if (lane < 16) atomicAdd(p.db + kBiasOther + col, bsum);
    }
}
#endif

}  // namespace cavoid
