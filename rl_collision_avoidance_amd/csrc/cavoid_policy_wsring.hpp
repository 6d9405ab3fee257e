// cavoid_policy_wsring.hpp -- NetworkVP_rnn with MULTI_AGENT_ARCH 'weight_sharing' for rows of 20..64 observed neighbours: the actors'
// predict_p_and_v + select_action (policy_wsring_forward_kernel<false>) and the trainer's forward pass with either loss head
// (policy_wsring_forward_kernel<true>, policy_wsring_regression_kernel).  The crowd step form's worlds (cavoid_crowd.hpp) observe up to 63
// neighbours; policy_ws_forward_tile (cavoid_policy_ws.hpp) parks the whole padded input row in LDS and stops at kWsMaxOthers = 19
// (80 + 16 + 8M + 8 <= 260).
//
// policy_wsring_tile<TRAIN, LOSS> is policy_ws_forward_tile<TRAIN, LOSS> with the R = kWsMaxOthers input slots at LDS columns
// kPolXCol + 8 + 8s used as a RING (what SpRing is to the LSTM inference kernel, cavoid_policy_crowd.hpp, and policy_train_ring_tile to its
// trainer pass, cavoid_policy_train_ring.hpp):
//   * same workgroup (64 rows, 4 wavefronts), same LDS buffer (policy_lds_bytes(4), stride kPolStride), same packed fragments and biases
//     (ws_layout(M) and policy_ws_pack_kernel hold for M <= 64: every fragment offset is int64_t, the largest k a pack thread forms is
//     16 * 1024 + 15), the filter MFMAs, policy_gemm per slot into the persistent layer1 accumulators, layer2 / fc1,
//     policy_heads<4, TRAIN, LOSS, false>, the row list, the action draw, policy_finish;
//   * staging parks the count, the host state and slots 0 .. min(M, R) - 1 -- the padded width stays 16 + 8 min(M, R) + 8 <= 176, inside
//     policy_div's range (the whole row, 536 at M = 64, is not); before slot i is processed ring slot i % R holds [xn_i (7) | is_on_i];
//   * slot i + R (when i + R < M) is loaded from global memory at the start of iteration i -- 64 rows x 8 values, two per thread, through
//     tile_row[] when a row list is given, with avg / std for the seven features -- normalised by the staging's own expression
//     (v - avg) / std, is_on by the staging's own comparison of the raw count (LDS column kPolXCol) with i + R + 1, and written into slot
//     i % R behind the loop's first barrier: by then every wavefront has read slot i.  The loop's second barrier publishes the write.
//     Tile rows at or past rows_here get zeros in all eight columns, as the staging leaves them;
//   * the last iteration's fifth K chunk (the host chunk at kPolXCol + 4) also reads ring slots 0 and 1, against zero weights: what is
//     parked there is finite as long as the input is.
// TRAIN leaves policy_ws_forward_kernel<true>'s memory contract to the byte -- l1_in [rows64, 4 + 64M], f_in[i] (copied from the ring slot
// during iteration i, not in one block at staging), z1..z3, gh, loss[2], the heads' part of db -- so policy_ws_backward_kernel runs behind
// it unchanged: it parks no input row, reads l1_in / z* / gh from global memory and forms every index that grows with M or the row count
// in int64_t (checked for M = 64 and 2^25 rows: row * w1, (i * rows64 + row) * 64 and i * kChWide * kFragPerChunkNarrow all are).
// On rows of <= R slots no ring slot is refilled before its last reader, and the kernels give bit for bit what the M <= 19 kernels give
// (tests/test_gpu_policy_wsring.py).
//
// Its own copy of policy_ws_forward_tile's lines, not a template parameter of it: the existing kernels keep their instruction streams
// whatever the compiler makes of a ring in that function (cavoid_policy_crowd.hpp and cavoid_policy_train_ring.hpp do the same).
//
// Not measured before this was written: at M = 64 the layer1 fragments are 257 chunks x 16 KB = 4.1 MB, past the "L2-resident" weight
// pack of M <= 19 (1.25 MB).  profiles/policy_wsring_timing.txt holds what that costs.
#pragma once
#ifndef CAVOID_POLICY_WS_LAYOUT_ONLY
#error "include with CAVOID_POLICY_WS_LAYOUT_ONLY: ws_layout, PolicyWsArgs and the constants of cavoid_policy_ws.hpp, none of its kernels"
#endif
#include "cavoid_policy_ws.hpp"

namespace cavoid {

constexpr int kWsMaxOthersCrowd = 64;          // the widest weight-sharing row (the env's own limit; ga3c/policy_kernel.py MAX_OTHERS_WS_CROWD)
constexpr int kWsRing = kWsMaxOthers;          // R: every input slot the LDS row has -- the fewest refills

template <bool TRAIN, int LOSS>
__device__ __forceinline__ void policy_wsring_tile(const PolicyWsArgs &wa) {
    constexpr int RT = 4, kRows = 64, R = kWsRing;
    const PolicyArgs &p = wa.a;
    // LDS: policy_ws_forward_tile's.  While the slots run, a row is
    //   cols 0..63 f_i (filter outputs of the current slot) | 80 raw num_other | 84..87 host | 88+8s..94+8s xn of the slot parked in ring
    //   slot s, 95+8s its is_on
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
    const int staged = M < R ? M : R;                      // slots the staging parks
    const int step = (!TRAIN && p.actions_out) ? *p.step_counter : 0;
    if (!TRAIN && p.row_index && rows_here == 0) {
        if (p.actions_out) policy_finish(p, step, tid);
        return;
    }
    const WsLayout L = ws_layout(M);
    const int w1 = kPolHost + kPolHidden * M;              // layer1's input width (TRAIN: the row stride of l1_in)

    // ---- input tile: gather + normalise the count, the host state and the first `staged` slots, is_on_i from the raw count --------
    if (!TRAIN && p.row_index) {
        if (tid < kRows) tile_row[tid] = tid < rows_here ? p.row_index[row0 + tid] : 0;
        __syncthreads();
    }
    const bool listed = !TRAIN && p.row_index != nullptr;
    const float *src = listed ? p.x : p.x + row0 * p.stride;
    {
        const int wpad = 16 + 8 * staged + 8;              // [num,0,0,0, host(4), staged x (xn_i(7), is_on_i), 16 zeros]
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
    if (ticket & 1) __builtin_amdgcn_s_setprio(1);
    if (TRAIN) {                                           // the host columns of layer1's input rows
        for (int e = tid; e < kRows * kPolHost; e += 256) {
            const int r = e >> 2, k = e & 3;
            p.l1_in[(row0 + r) * w1 + k] = act[r * kPolStride + kPolXCol + 4 + k];
        }
    }

    // the ring's element e = tid + 256 u of one slot's 64 x 8 values -- tile row e / 8, column e % 8 (7: is_on).  ring_src: the row's
    // first float in global memory, -1 for a tile row at or past rows_here (zeros); ring_cnt: the row's raw count
    int ring_lds[2], ring_k[2];
    int64_t ring_src[2];
    float ring_cnt[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int e = tid + 256 * u, r = e >> 3;
        ring_k[u] = e & 7;
        ring_lds[u] = r * kPolStride + kPolXCol + 8 + ring_k[u];
        ring_src[u] = r < rows_here ? (int64_t)(listed ? tile_row[r] : r) * p.stride : -1;
        ring_cnt[u] = act[r * kPolStride + kPolXCol];
    }

    // ---- the slots: filter, then the slot's 4 K chunks of layer1 into the persistent accumulators -----------------------
    f32x4 acc[RT][4];
    policy_init_acc(lds_bias + kBiasL1, 4 * wave, lane, acc);
    const f32x4 fw = p.frags[L.filter + 64 * wave + lane];  // filter weights of this wavefront's 16 units (one K chunk)
    const float fb = lds_bias[kBiasOther + 16 * wave + (lane & 15)];
    const float *arow = act + (lane & 15) * kPolStride + 4 * (lane >> 4);
    float *frow = act + (4 * (lane >> 4)) * kPolStride + 16 * wave + (lane & 15);
    PolicyFrag<RT, 4> f0;
    int slot = 0;                                          // i % R
    for (int i = 0; i < M; ++i) {
        const f32x4 *l1 = p.frags + L.l1 + (int64_t)4 * i * kFragPerChunk;
        policy_load_b(f0, l1, 4 * wave, lane, 0);          // in flight across the filter and the barriers
        // slot i + R into registers (uniform): in flight across the filter MFMAs and the first barrier
        const bool refill = i + R < M;
        float rv[2], rav[2], rsd[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int sc = 1 + kPolHost + kPolOther * (i + R) + ring_k[u];
            const bool in = refill && ring_src[u] >= 0 && ring_k[u] < kPolOther;
            rv[u] = in ? src[ring_src[u] + sc] : 0.0f;
            const bool norm = in && p.avg != nullptr;
            rav[u] = norm ? p.avg[sc] : 0.0f;
            rsd[u] = norm ? p.std[sc] : 1.0f;
        }
        const int scol = kPolXCol + 8 + 8 * slot;
        if (TRAIN) {                                       // the slot's filter input rows, for the filter's weight gradient
#pragma unroll
            for (int u = 0; u < 2; ++u)
                wa.f_in[((int64_t)i * p.rows64 + row0 + ((tid + 256 * u) >> 3)) * kWsFilterIn + ring_k[u]] = act[ring_lds[u] + 8 * slot];
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
        __syncthreads();                                   // every wavefront has read f_{i-1} and ring slot i % R
        if (refill) {
            const float thr = (float)(i + R + 1);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float on = ring_src[u] >= 0 && ring_cnt[u] >= thr ? 1.0f : 0.0f;
                act[ring_lds[u] + 8 * slot] = ring_k[u] == kPolOther ? on : (rv[u] - rav[u]) / rsd[u];
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
        __syncthreads();                                   // f_i and the refilled slot are in place
        // the last slot also takes the host chunk (chunk 4 reads the host columns, as layer1 of the LSTM kernel does)
        policy_gemm(act, l1, 0, i + 1 < M ? 4 : 5, kPolXCol + 4, 4 * wave, lane, f0, acc);
        slot = slot + 1 == R ? 0 : slot + 1;
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
    policy_heads<RT, TRAIN, LOSS, false>(p, act, lds_bias, p.frags + L.head, hb, tile_row, listed, row0, rows_here, step, wave, lane);
    if (!TRAIN && p.actions_out) policy_finish(p, step, tid);
}

#ifdef CAVOID_POLICY_WSRING_KERNELS     /* compiled by cavoid_policy_wsring.hip only */
template <bool TRAIN>
__global__ void __launch_bounds__(256, TRAIN ? 1 : 2) policy_wsring_forward_kernel(const PolicyWsArgs wa) {
    policy_wsring_tile<TRAIN, kLossA3C>(wa);
}

// the supervised start's pass (cavoid_policy_train_regression_ws on a _create_ws_crowd handle): the same forward with the regression head
__global__ void __launch_bounds__(256, 1) policy_wsring_regression_kernel(const PolicyWsArgs wa) {
    policy_wsring_tile<true, kLossRegression>(wa);
}
#endif

}  // namespace cavoid
