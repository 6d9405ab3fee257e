// cavoid_policy_crowd.hpp -- the actors' NetworkVP_rnn inference (predict_p_and_v + select_action) for rows of 20..64 observed agents: the crowd
// step form's worlds (cavoid_crowd.hpp) observe up to 63 neighbours, the stand-alone split kernel (cavoid_policy_split.hpp) parks a whole input
// row in LDS and stops at kSpMaxOthers = 23 (kPolMaxOthers = 19 for every form).
//
// policy_crowd_forward_kernel<P> is policy_forward_split_kernel<P> with the input slots used as a RING (policy_split_tile's SpRing):
//   * same workgroup (64 rows, 4 wavefronts), same two 16-bit activation planes (70 KB of LDS: 2 workgroups per CU), same per-step GEMM over
//     [h | input slot] and per-lane cell update, same heads, row list, action draw and launch counter;
//   * staging parks the host slot and observed agents 0 .. R-1 (slots 1 .. R, R = kSpCrowdRing); before LSTM step t slot 1 + t % R holds agent t;
//   * agent t + R is fetched from global memory at the start of step t (elements 2w, 2w + 1 by wavefront w, one tile row per lane: 2 values and,
//     with NORMALIZE_INPUT, their avg / std), i.e. while step t's matrix instructions run, and normalised, split and written into slot 1 + t % R
//     behind the barrier that ends step t's GEMM -- the next reader of that slot is step t + R.
// The staging's statements on the same values: a row of <= R observed agents gives bit for bit what the split kernel gives it
// (tests/test_gpu_policy_crowd.py).  Two product forms: kSpF16 (the default) and 3 (bf16 pieces: float32's range, cavoid_policy_info).
#pragma once
#include "cavoid_policy_split.hpp"

namespace cavoid {

constexpr int kPolMaxOthersInference = 64;      // the widest row cavoid_policy_create / _forward take (the env's own limit, 64 agents per world)
constexpr int kPolCrowdMaxStride = 1 + 6 + kPolOther * kPolMaxOthersInference;   // row stride limit of a crowd handle: the widest env observation row
constexpr int kSpCrowdRing = kSpMaxOthers;      // R: every slot column the planes have (64 + 8 R + 7 <= 255) -- the fewest refills

// policy_forward_split_kernel's workgroup with the Ring.  (Its own copy of those lines: the split kernel's body moved into a shared inline
// function compiles to a differently scheduled instruction stream, and the existing kernels stay as they were.)
// Occupancy: the default form fits 256 registers, 2 workgroups per CU (the LDS allows 2); the bf16 form's third register group (its slot
// chunk is three products, not one mixed one) spills 118 registers to scratch at 256, so it runs 1 workgroup per CU with 332 and no scratch.
// (Named policy_crowd_forward_kernel: names ending in "crowd_kernel" are the env's crowd step kernels.)
template <int P>
__global__ void __launch_bounds__(256, P == kSpF16 ? 2 : 1) policy_crowd_forward_kernel(const SplitArgs sa) {
    const PolicyArgs &p = sa.p;
    extern __shared__ __attribute__((aligned(16))) unsigned char planes[];      // plane 1 (hi), plane 2 (lo)
    float *len_f = reinterpret_cast<float *>(planes + 2 * kSpPlaneB);            // [64] raw num_other_agents
    int *tile_row = reinterpret_cast<int *>(len_f + 64);                          // [64] global row of each tile row
    int *wave_max = tile_row + 64;                                                // [4] + ticket
    int &ticket = wave_max[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t row0 = (int64_t)blockIdx.x * 64;
    const int64_t n_rows = p.row_count ? (int64_t)*p.row_count : p.rows;
    const int rows_here = n_rows - row0 < 64 ? (int)(n_rows - row0 > 0 ? n_rows - row0 : 0) : 64;
    const int A = p.num_actions;
    const int step = p.actions_out ? *p.step_counter : 0;
    const bool listed = p.row_index != nullptr;
    if (listed && rows_here == 0) {                        // uniform over the workgroup: nothing listed for this tile
        if (p.actions_out) policy_finish(p, step, tid);
        return;
    }
    if (tid < 64) tile_row[tid] = listed ? (tid < rows_here ? p.row_index[row0 + tid] : 0) : tid;   // row of `src` behind each tile row
    if (tid == 0) ticket = policy_cu_ticket(p.cu_tickets);   // arrival parity on the CU -> static priority (policy_cu_ticket, cavoid_policy.hpp)
    __syncthreads();
    if (ticket & 1) __builtin_amdgcn_s_setprio(1);
    const float *src = listed ? p.x : p.x + row0 * p.stride;
    // (rows past rows_here are never read: the staging and the ring's fetch take row 0 for them)
    auto load = [&](int r, int k) -> float { return src[(int64_t)tile_row[r] * p.stride + k]; };
    auto emit = [&](int trow, int g, const float (&pj)[4], const f32x4 &logit) {
        const bool in_tile = trow < rows_here;
        const int64_t row = listed ? (in_tile ? (int64_t)tile_row[trow] : p.rows) : row0 + trow;
        if (row < p.rows) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = 4 * g + r;
                if (col < A) p.p_out[row * A + col] = pj[r];
                else if (col == A) p.v_out[row] = logit[r];
            }
        }
        if (p.actions_out) {                               // wave-uniform
            const int action = split_select_action(pj, g, lane, A, p.greedy != 0, row, step, p.seed_lo, p.seed_hi);
            if (row < p.rows && g == 0) p.actions_out[row] = action;
        }
    };
    policy_split_tile<P, 0, false, SpRing<kSpCrowdRing>>(sa, planes, len_f, wave_max, rows_here, tid, load, emit);
    if (p.actions_out) policy_finish(p, step, tid);
}

}  // namespace cavoid
