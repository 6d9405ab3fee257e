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

// The heads and what follows them (softmax + MIN_POLICY, outputs, A3C loss and its gradient, action draw): the epilogue of
// policy_forward_kernel<4, TRAIN>, marked copy (that kernel keeps its instruction stream).  hb[0 .. 8) is loaded by the caller.
// LOSS (TRAIN only): kLossA3C, or kLossRegression -- policy_regression_head, the one copy both networks share.
template <bool TRAIN, int LOSS>
__device__ __forceinline__ void policy_ws_heads(const PolicyArgs &p, const float *act, const float *lds_bias, const f32x4 *head,
                                                f32x4 (&hb)[kChHead], const int *tile_row, bool listed, int64_t row0, int rows_here,
                                                int step, int wave, int lane) {
    constexpr int RT = 4;
    if (wave >= RT) return;
    f32x4 acc[4];
    const float b = lds_bias[kBiasHead + (lane & 15)];
    acc[0] = f32x4{b, b, b, b};
    acc[1] = acc[2] = acc[3] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *arow = act + (16 * wave + (lane & 15)) * kPolStride + 4 * (lane >> 4);
#pragma unroll
    for (int g = 0; g < kChHead; g += 4) {
        if (g == 0) {
#pragma unroll
            for (int ch = kChHead / 2; ch < kChHead; ++ch) hb[ch] = head[lane + 64 * ch];
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
        const int trow = 16 * wave + 4 * (lane >> 4) + r;
        const bool in_tile = TRAIN || trow < rows_here;
        const int64_t row = listed ? (in_tile ? (int64_t)tile_row[trow] : p.rows) : row0 + trow;
        const float sm = e / sum;
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
            const bool valid = row < p.rows;
            const float y = valid ? p.y_r[row] : 0.0f;
            const int a = valid ? p.a_idx[row] : 0;
            const float v = __shfl(z, A, 16);
            const float sel = __shfl(pj, a, 16);
            const float lp = __logf(fmaxf(pj, p.log_eps));
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
        if (!TRAIN && p.actions_out) {
            int action;
            if (p.greedy) {
                float best = pj;
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) best = fmaxf(best, __shfl_xor(best, d, 16));
                int idx = (col < A && pj == best) ? col : 99;
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) { const int o = __shfl_xor(idx, d, 16); idx = o < idx ? o : idx; }
                action = idx;
            } else {
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
    if (TRAIN) {
        cost_p += __shfl_xor(cost_p, 16, 64); cost_p += __shfl_xor(cost_p, 32, 64);
        cost_v += __shfl_xor(cost_v, 16, 64); cost_v += __shfl_xor(cost_v, 32, 64);
        if (lane == 0) { atomicAdd(p.loss, cost_p); atomicAdd(p.loss + 1, cost_v); }
        gsum += __shfl_xor(gsum, 16, 64); gsum += __shfl_xor(gsum, 32, 64);
        if (lane < 16) atomicAdd(p.db + kBiasHead + lane, gsum);
    }
}

// The forward pass of one tile is ONE text, cavoid_policy_ws_forward_body.hpp, compiled into both kernels below: they differ in the
// loss head alone (LOSS).  Included, not called, for the reason given at policy_forward_kernel (cavoid_policy.hpp).
template <bool TRAIN>
__global__ void __launch_bounds__(256, TRAIN ? 1 : 2) policy_ws_forward_kernel(const PolicyWsArgs wa) {
    constexpr int LOSS = kLossA3C;
#include "cavoid_policy_ws_forward_body.hpp"
}

// The supervised start's trainer pass (cavoid_policy_train_regression_ws): the TRAIN forward with the regression head.  It leaves
// what policy_ws_forward_kernel<true> leaves, so that policy_ws_backward_kernel runs behind it unchanged.
__global__ void __launch_bounds__(256, 1) policy_regression_ws_forward_kernel(const PolicyWsArgs wa) {
    constexpr bool TRAIN = true;
    constexpr int LOSS = kLossRegression;
#include "cavoid_policy_ws_forward_body.hpp"
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
    {
        f32x4 acc[RT][4];
        policy_zero_acc(acc);
        policy_gemm(act, p.frags + L.thead, 0, 1, 64, 4 * wave, lane, f0, acc);
        policy_load_b(f0, p.frags + L.tfc1, 4 * wave, lane, 0);
        __syncthreads();
        policy_store_masked(act, 4 * wave, lane, acc, p.z3 + row0 * kPolWidth, p.g3 + row0 * kPolWidth, p.db + kBiasFc1);
        __syncthreads();
    }
    {
        f32x4 acc[RT][4];
        policy_zero_acc(acc);
        policy_gemm(act, p.frags + L.tfc1, 0, kChWide, 64, 4 * wave, lane, f0, acc);
        policy_load_b(f0, p.frags + L.tl2, 4 * wave, lane, 0);
        __syncthreads();
        policy_store_masked(act, 4 * wave, lane, acc, p.z2 + row0 * kPolWidth, p.g2 + row0 * kPolWidth, p.db + kBiasL2);
        __syncthreads();
    }
    {
        f32x4 acc[RT][4];
        policy_zero_acc(acc);
        policy_gemm(act, p.frags + L.tl2, 0, kChWide, 64, 4 * wave, lane, f0, acc);
        __syncthreads();
        policy_store_masked(act, 4 * wave, lane, acc, p.z1 + row0 * kPolWidth, p.g1 + row0 * kPolWidth, p.db + kBiasL1);
        __syncthreads();
    }
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

}  // namespace cavoid
