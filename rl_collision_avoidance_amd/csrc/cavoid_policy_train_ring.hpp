// cavoid_policy_train_ring.hpp -- the trainer's forward pass (forward + loss head + gradient at the heads) of NetworkVP_rnn for rows of
// 20..64 observed agents: the crowd step form's worlds (cavoid_crowd.hpp) observe up to 63 neighbours, policy_forward_kernel<4, true>
// (cavoid_policy.hpp) parks the whole padded input row in LDS and stops at kPolMaxOthers = 19 (80 + 16 + 8M + 8 <= 260).
//
// policy_train_ring_forward_kernel / policy_train_ring_regression_kernel are policy_forward_kernel<4, true> / policy_regression_forward_kernel<4>
// with the R = kPolMaxOthers input slots at LDS columns kPolXCol + 8 + 8s used as a RING (what SpRing is to the inference kernel,
// cavoid_policy_crowd.hpp):
//   * same workgroup (64 rows, 4 wavefronts), same LDS buffer (policy_lds_bytes(4), stride kPolStride, h / num_other / host columns), same
//     packed fragments and biases, policy_gemm, per-lane cell update (with its fence on keep / add), policy_heads<4, true, LOSS, false>;
//   * staging parks the host state and observed agents 0 .. min(M, R) - 1 -- the padded width stays 16 + 8 min(M, R) + 8 <= 176, inside
//     policy_div's range (the whole row, 536 at M = 64, is not); before LSTM step t slot t % R holds agent t;
//   * agent t + R (when a row of the tile runs step t + R) is loaded from global memory at the start of step t -- 64 rows x 7 values, at most
//     2 per thread, with their avg / std -- i.e. while step t's matrix instructions run, normalised by the staging's own expression
//     (v - avg) / std, and written into slot t % R behind the barrier that ends step t's GEMM; the step's second barrier publishes it, and
//     the slot's next readers are step t + R (its x_t) and step t + R - 1 (the upper half of its 16-wide input chunk: zero weights);
//   * step t's GEMM and its h_in[t] record read slot t % R.
// What they leave in memory is policy_forward_kernel<4, true>'s contract to the byte -- z1..z3, l1_in, h_in[t], the save records at
// (blockIdx.x * M + t), gh, loss[2], the heads' part of db -- so policy_backward_kernel<4> runs behind them unchanged: it walks
// t = M-1 .. 0 over those records in global memory and parks no input row.  Every index into save / h_in (and the backward's into gl) is
// formed in int64_t: at M = 64 and 2^25 rows the save index passes 2^31 records.
// On rows of <= R observed agents no slot is refilled before its last reader, and the kernels give bit for bit what the M <= 19 kernels
// give (tests/test_gpu_policy_train_ring.py).
//
// Its own copy of policy_forward_tile's lines (RT = 4, TRAIN), not a template parameter of it: the existing kernels keep their instruction
// streams whatever the compiler makes of a ring in that function (cavoid_policy_crowd.hpp does the same for the same reason).  The
// development build's phase stamps (CAVOID_TRACE) are left out.
#pragma once
#include "cavoid_policy.hpp"

namespace cavoid {

constexpr int kPolMaxOthersTrain = 64;          // the widest row the trainer pass takes (the env's own limit; ga3c/policy_kernel.py MAX_OTHERS_TRAIN)
constexpr int kPolTrainRing = kPolMaxOthers;    // R: every input slot the LDS row has -- the fewest refills

template <int LOSS>
__device__ __forceinline__ void policy_train_ring_tile(const PolicyArgs &p) {
    constexpr int RT = 4, kRows = 16 * RT, R = kPolTrainRing;
    // LDS: policy_forward_tile's.  While the LSTM runs, a row is
    //   cols 0..63 h | 80 raw num_other | 84..87 host | 88+8s..94+8s the agent in ring slot s (column 95+8s: 0), zeros up to 255
    extern __shared__ __attribute__((aligned(16))) float act[];
    float *lds_bias = act + kRows * kPolStride;
    int *wave_max = reinterpret_cast<int *>(lds_bias + kBiasFloats);
    int &ticket = wave_max[4];
    int *tile_row = wave_max + 8;                          // (policy_heads' argument: unused without a row list)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t row0 = (int64_t)blockIdx.x * kRows;
    const int rows_here = p.rows - row0 < kRows ? (int)(p.rows - row0 > 0 ? p.rows - row0 : 0) : kRows;
    const int M = p.max_other;
    const int staged = M < R ? M : R;                      // agents the staging parks
    const f32x4 *w_lstm = p.frags + kOffLstm;
    PolicyFrag<RT, 4> f0;
    policy_load_b(f0, w_lstm, 4 * wave, lane, 4);          // first LSTM step: h == 0, only the input chunk contributes
    const float *src = p.x + row0 * p.stride;              // (never read for tile rows >= rows_here)

    // ---- input tile: gather + normalise the host state and the first `staged` agents into the padded layout above -----------
    {
        const int wpad = 16 + 8 * staged + 8;              // padded row: [num,0,0,0, host(4), staged x (x_t(7),0), 16 zeros]
        const float inv_wpad = 1.0f / (float)wpad;
        const int total = kRows * wpad;
        constexpr int U = 3 * RT;
        int local_max = 0;
        float bias_v[(kBiasFloats + 255) / 256];
#pragma unroll
        for (int u = 0; u < (kBiasFloats + 255) / 256; ++u) bias_v[u] = tid + 256 * u < kBiasFloats ? p.bias[tid + 256 * u] : 0.0f;
        if (tid == 0) {                                    // arrival parity on the CU -> static priority (see policy_forward_tile)
            const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
            const uint32_t key = ((xcc & 15u) << 8) | ((hw >> 8) & 0xFFu);
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
                else if (c >= 8 && c < 8 + 8 * staged && (c & 7) != 7) sc = 1 + kPolHost + kPolOther * ((c - 8) >> 3) + (c & 7);
                const bool in = e < total && sc >= 0 && r < rows_here;
                dst[u] = e < total ? r * kPolStride + kPolXCol + c : -1;
                v[u] = in ? src[(int64_t)r * p.stride + sc] : 0.0f;
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
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_xor(local_max, d, 64); local_max = o > local_max ? o : local_max; }
        if (lane == 0) wave_max[wave] = local_max;
    }
    __syncthreads();
    const int m01 = wave_max[0] > wave_max[1] ? wave_max[0] : wave_max[1], m23 = wave_max[2] > wave_max[3] ? wave_max[2] : wave_max[3];
    const int steps = m01 > m23 ? m01 : m23;               // LSTM steps any row of this tile still needs (<= M)
    if (ticket & 1) __builtin_amdgcn_s_setprio(1);

    // this lane's rows in the C layout and their sequence lengths
    float len_r[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) len_r[rt][r] = act[(16 * rt + 4 * (lane >> 4) + r) * kPolStride + kPolXCol];

    // the ring's refill: element e = tid + 256 u of the 64 x 7 values of one agent -- tile row e / 7, input e % 7
    int ring_dst[2], ring_row[2], ring_k[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int e = tid + 256 * u;
        ring_row[u] = e / kPolOther; ring_k[u] = e - ring_row[u] * kPolOther;
        const bool mine = e < kRows * kPolOther && ring_row[u] < rows_here;
        if (!mine) ring_row[u] = -1;
        ring_dst[u] = e < kRows * kPolOther ? (e / kPolOther) * kPolStride + kPolXCol + 8 + ring_k[u] : -1;
    }

    // ---- LSTM over the observed agents -------------------------------------------------------------------
    f32x4 cell[RT], hid[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) { cell[rt] = f32x4{0.f, 0.f, 0.f, 0.f}; hid[rt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    int slot = 0;                                          // t % R
    for (int t = 0; t < steps; ++t) {
        // agent t + R into registers (uniform: only when a row of the tile runs step t + R; t + R < steps <= M)
        const bool refill = t + R < steps;
        float rv[2], rav[2], rsd[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int sc = 1 + kPolHost + kPolOther * (t + R) + ring_k[u];
            const bool in = refill && ring_row[u] >= 0;
            rv[u] = in ? src[(int64_t)ring_row[u] * p.stride + sc] : 0.0f;
            const bool norm = in && p.avg != nullptr;
            rav[u] = norm ? p.avg[sc] : 0.0f;
            rsd[u] = norm ? p.std[sc] : 1.0f;
        }
        const int xcol = kPolXCol + 8 + 8 * slot;
        {                                                  // the step's input rows, for the LSTM weight gradient
            float *dst = p.h_in + ((int64_t)t * p.rows64 + row0) * 72;
            for (int e = tid; e < kRows * 72; e += 256) {
                const int r = e / 72, k = e - r * 72;
                dst[e] = k < kPolHidden ? act[r * kPolStride + k]
                                        : (k < kPolHidden + kPolOther ? act[r * kPolStride + xcol + (k - kPolHidden)] : 0.0f);
            }
        }
        f32x4 acc[RT][4];
        policy_init_acc(lds_bias + kBiasLstm, 4 * wave, lane, acc);
        policy_gemm(act, w_lstm, t == 0 ? 4 : 0, kChLstm, xcol, 4 * wave, lane, f0, acc);
        policy_load_b(f0, w_lstm, 4 * wave, lane, 0);      // the next step's first weight fragments
        __syncthreads();                                   // every wavefront has read h and the input slots
        if (refill) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
                if (ring_dst[u] >= 0) act[ring_dst[u] + 8 * slot] = (rv[u] - rav[u]) / rsd[u];
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // dynamic_rnn: rows past their own length keep (c, h) -- selects, not branches
                const bool live = len_r[rt][r] > (float)t;
                const float gi = fast_sigmoid(acc[rt][0][r]), gj = fast_tanh(acc[rt][1][r]);
                const float gf = fast_sigmoid(acc[rt][2][r]), go = fast_sigmoid(acc[rt][3][r]);
                float keep = gf * cell[rt][r], add = gi * gj;
                asm volatile("" : "+v"(keep), "+v"(add));  // (no packed add with swapped halves: DESIGN.md 3.7 (d))
                const float c_new = keep + add;
                const float tc = fast_tanh(c_new);
                const float h_new = go * tc;
                // lane-private 32-byte records: the backward pass reads them back as is
                f32x4 *sv = reinterpret_cast<f32x4 *>(p.save) + ((((int64_t)blockIdx.x * M + t) * 16 + (rt * 4 + r)) * 256 + tid) * 2;
                sv[0] = f32x4{gi, gj, gf, go};
                sv[1] = f32x4{cell[rt][r], tc, 0.0f, 0.0f};
                cell[rt][r] = live ? c_new : cell[rt][r];
                hid[rt][r] = live ? h_new : hid[rt][r];
                act[(16 * rt + 4 * (lane >> 4) + r) * kPolStride + 16 * wave + (lane & 15)] = hid[rt][r];
            }
        __syncthreads();                                   // the new h and the refilled slot are in place
        slot = slot + 1 == R ? 0 : slot + 1;
    }
    // ---- layer1 on [h | host] --------------------------------------------------------------------------------
    {
        float *dst = p.l1_in + row0 * 72;                  // layer1's input rows [h | host | 0], for its weight gradient
        for (int e = tid; e < kRows * 72; e += 256) {
            const int r = e / 72, k = e - r * 72;
            dst[e] = k < kPolHidden ? act[r * kPolStride + k]
                                    : (k < kPolHidden + kPolHost ? act[r * kPolStride + kPolXCol + 4 + (k - kPolHidden)] : 0.0f);
        }
        f32x4 acc[RT][4];
        policy_load_b(f0, p.frags + kOffL1, 4 * wave, lane, 0);
        policy_init_acc(lds_bias + kBiasL1, 4 * wave, lane, acc);
        policy_gemm(act, p.frags + kOffL1, 0, kChL1, kPolXCol + 4, 4 * wave, lane, f0, acc);
        policy_load_b(f0, p.frags + kOffL2, 4 * wave, lane, 0);
        __syncthreads();
        policy_store_relu(act, 4 * wave, lane, acc, p.z1 + row0 * kPolWidth);
        __syncthreads();
    }
    // ---- layer2, fullyconnected1 -----------------------------------------------------------------------------
    {
        f32x4 acc[RT][4];
        policy_init_acc(lds_bias + kBiasL2, 4 * wave, lane, acc);
        policy_gemm(act, p.frags + kOffL2, 0, kChWide, 64, 4 * wave, lane, f0, acc);
        policy_load_b(f0, p.frags + kOffFc1, 4 * wave, lane, 0);
        __syncthreads();
        policy_store_relu(act, 4 * wave, lane, acc, p.z2 + row0 * kPolWidth);
        __syncthreads();
    }
    f32x4 hb[kChHead];                                     // the heads' weight fragments: half here, half in policy_heads
    {
        f32x4 acc[RT][4];
        policy_init_acc(lds_bias + kBiasFc1, 4 * wave, lane, acc);
        policy_gemm(act, p.frags + kOffFc1, 0, kChWide, 64, 4 * wave, lane, f0, acc);
        const f32x4 *brow = p.frags + kOffHead + lane;
        __syncthreads();
        policy_store_relu(act, 4 * wave, lane, acc, p.z3 + row0 * kPolWidth);
        __syncthreads();
#pragma unroll
        for (int ch = 0; ch < kChHead / 2; ++ch) hb[ch] = brow[64 * ch];
    }
    policy_heads<RT, true, LOSS, false>(p, act, lds_bias, p.frags + kOffHead, hb, tile_row, false, row0, rows_here, 0, wave, lane);
}

#ifdef CAVOID_POLICY_TRAIN_RING_KERNELS     /* compiled by cavoid_policy_train_ring.hip only */
__global__ void __launch_bounds__(256, 1) policy_train_ring_forward_kernel(const PolicyArgs p) {
    policy_train_ring_tile<kLossA3C>(p);
}

// the supervised start's pass (cavoid_policy_train_regression on a crowd handle): the same forward with the regression head
__global__ void __launch_bounds__(256, 1) policy_train_ring_regression_kernel(const PolicyArgs p) {
    policy_train_ring_tile<kLossRegression>(p);
}
#endif

}  // namespace cavoid
