// cavoid_policy_step_ws.hpp -- the rest of the trainer step for the WEIGHT-SHARING network, behind cavoid_policy_weight_grads_ws /
// cavoid_policy_apply_ws (include/cavoid.h):
//   step_ws_gemm_kernel    the five contractions X^T G of cavoid_policy_train_ws's buffers on the tiles of cavoid_policy_step.hpp, cut into
//                          row slices: one wavefront forms one tile of one slice's partial product, straight from the pass's buffers;
//   step_ws_reduce_kernel  sums every entry's partials in slice order into the flat gradient vector (cavoid_policy_param_layout_ws),
//                          moves db into the six biases and zeroes the padding.
// The optimiser is step_norm_kernel / step_apply_kernel of cavoid_policy_step.hpp themselves: they take the layout as an argument
// (cavoid_policy_step_update).
// Nothing is permuted: l1_in's columns [host 4 | f_0 .. f_{M-1}] and f_in's [xn 7 | is_on] are the checkpoint's row orders, so the
// partials are in the checkpoint's layout already.  layer1 = l1_in^T g1 is M + 1 row blocks of the [4 + 64 M, 256] product: the 64-column
// block of slot i starts at column 4 + 64 i of a row of 16 (1 + 16 M) bytes -- 16-byte aligned, step_gemm_44 as it is -- and the host
// columns 0..3 are an edge tile with 4 live columns; other_kernel = f_in^T gf over the flat max_other * rows rows is an edge tile with 8.
// The partition depends on the buffer rows and max_other only, nothing uses a floating-point atomic: the same buffers give the same bits.
#pragma once
#include "cavoid_policy_step.hpp"

namespace cavoid {

// the row slices.  A tile's loop is one step of 4 rows deep, so a wavefront alone on its SIMD waits out every load: short slices --
// several wavefronts per SIMD -- are what hides that.  layer1 therefore keeps the dense jobs' 1 024 rows although its partial is
// [4 + 64 M, 256] floats (4 MB at M = 63, 66 MB of partials at 16 384 rows, a tenth of what the pass itself keeps there): with slices of
// 4 096 rows from M = 25 on and for the filter from 65 536 flat rows on, as first built, cavoid_policy_weight_grads_ws took 600 to 800 us
// at every shape of profiles/policy_ws_device_step_timing.txt -- the time of ONE 4 096-row tile.  The filter's flat M * rows rows are
// cut like the LSTM's.
constexpr int64_t kStepWsL1Slice = 1024;         // rows of l1_in / g1 per slice
constexpr int64_t kStepWsFilterSlice = 1024;     // rows of the flat [max_other * rows] filter operands per slice ...
constexpr int64_t kStepWsFilterSliceWide = 4096; // ... once there are more than kStepWsFilterWideFrom of them
constexpr int64_t kStepWsFilterWideFrom = 4194304;
constexpr int kStepWsFilterIn = 8;               // f_in's width: [xn 7 | is_on]
// one dense slice's partials (kStepDenseSlice rows): fullyconnected1 [256, 256] | layer2 [256, 256] | heads [256, 16]
constexpr int64_t kStepWsOffFc1 = 0, kStepWsOffL2 = 65536, kStepWsOffHead = 131072;
constexpr int64_t kStepWsDensePartial = kStepWsOffHead + kStepW * kStepHeads;
constexpr int64_t kStepWsFilterPartial = kStepWsFilterIn * kStepH;              // [8, 64]
constexpr int kStepWsDenseJobs = 16 + 16 + 4;

struct StepWsPartition { int64_t dense_slices, l1_len, l1_slices, f_len, f_slices; };
__host__ __device__ inline StepWsPartition step_ws_partition(int64_t rows, int32_t max_other) {
    StepWsPartition p;
    const int64_t t = rows * max_other;
    p.dense_slices = (rows + kStepDenseSlice - 1) / kStepDenseSlice;
    p.l1_len = kStepWsL1Slice;
    p.l1_slices = (rows + p.l1_len - 1) / p.l1_len;
    p.f_len = t > kStepWsFilterWideFrom ? kStepWsFilterSliceWide : kStepWsFilterSlice;
    p.f_slices = (t + p.f_len - 1) / p.f_len;
    return p;
}
inline int64_t step_ws_l1_partial(int32_t max_other) { return (int64_t)(kStepHost + kStepH * max_other) * kStepW; }
// scratch: the layer1 partials, then the dense ones, then the filter's
inline int64_t step_ws_scratch_floats(int64_t rows, int32_t max_other) {
    const StepWsPartition p = step_ws_partition(rows, max_other);
    return p.l1_slices * step_ws_l1_partial(max_other) + p.dense_slices * kStepWsDensePartial + p.f_slices * kStepWsFilterPartial;
}

// the flat parameter vector (cavoid_policy_param_layout_ws)
inline StepLayout step_ws_layout(int32_t max_other, int32_t num_actions) {
    const int64_t sizes[kStepParams] = {kStepWsFilterIn * kStepH, kStepH, (kStepHost + (int64_t)kStepH * max_other) * kStepW, kStepW, kStepW * kStepW, kStepW,
                                        kStepW * kStepW, kStepW, (int64_t)kStepW * num_actions, num_actions, kStepW, 1};
    StepLayout l;
    int64_t o = 0;
    for (int i = 0; i < kStepParams; ++i) {
        l.off[i] = o; l.size[i] = sizes[i]; l.total = o + sizes[i];
        o = (l.total + kStepAlign - 1) / kStepAlign * kStepAlign;
    }
    return l;
}

struct StepWsGemmArgs {
    const float *z1, *z2, *z3, *l1_in, *f_in, *gh, *g1, *g2, *g3, *gf;
    float *scratch;
    int64_t rows, f_rows;                        // buffer rows; max_other * buffer rows
    int64_t dense_slices, l1_len, l1_slices, f_len, f_slices;
    int32_t max_other;
};

struct StepWsReduceArgs {
    const float *scratch, *db;
    float *grads;
    int64_t off[kStepParams], size[kStepParams], total;
    int64_t dense_slices, l1_slices, f_slices, l1_partial;
    int32_t num_actions;
};

#ifdef CAVOID_POLICY_STEP_WS_KERNELS

// grid: l1_slices * 4 (max_other + 1) + dense_slices * kStepWsDenseJobs + f_slices workgroups of ONE wavefront (the longest jobs first)
__global__ __launch_bounds__(64) void step_ws_gemm_kernel(const StepWsGemmArgs a) {
    const int lane = threadIdx.x;
    const int M = a.max_other, ld1 = kStepHost + kStepH * M, l1_jobs = 4 * (M + 1);
    const int64_t l1_blocks = a.l1_slices * l1_jobs, dense_blocks = a.dense_slices * kStepWsDenseJobs;
    const int64_t l1_partial = (int64_t)ld1 * kStepW;
    int64_t b = blockIdx.x;
    if (b < l1_blocks) {                                           // layer1 = l1_in^T g1: row block (slot, or the host edge) x column block
        const int64_t s = b / l1_jobs, r0 = s * a.l1_len;
        const int j = (int)(b % l1_jobs), i = j >> 2, tg = j & 3;
        const int64_t n = (a.rows - r0 < a.l1_len) ? a.rows - r0 : a.l1_len;
        const float *x = a.l1_in + r0 * ld1, *g = a.g1 + r0 * kStepW + 64 * tg;
        float *part = a.scratch + s * l1_partial + 64 * tg;
        if (i < M) step_gemm_44(x + kStepHost + 64 * i, ld1, g, kStepW, n, part + (int64_t)(kStepHost + 64 * i) * kStepW, kStepW, lane);
        else step_gemm_edge<kStepHost>(x, ld1, g, kStepW, n, part, kStepW, lane);
        return;
    }
    b -= l1_blocks;
    if (b < dense_blocks) {
        const int64_t s = b / kStepWsDenseJobs, r0 = s * kStepDenseSlice;
        const int j = (int)(b % kStepWsDenseJobs);
        const int64_t n = (a.rows - r0 < kStepDenseSlice) ? a.rows - r0 : kStepDenseSlice;
        float *part = a.scratch + a.l1_slices * l1_partial + s * kStepWsDensePartial;
        if (j < 32) {                                              // fullyconnected1 = z2^T g3, layer2 = z1^T g2: 4 x 4 tiles each
            const float *x = (j < 16 ? a.z2 : a.z1) + r0 * kStepW, *g = (j < 16 ? a.g3 : a.g2) + r0 * kStepW;
            const int tx = (j & 15) >> 2, tg = j & 3;
            step_gemm_44(x + 64 * tx, kStepW, g + 64 * tg, kStepW, n, part + (j < 16 ? kStepWsOffFc1 : kStepWsOffL2) + (int64_t)64 * tx * kStepW + 64 * tg,
                         kStepW, lane);
        } else {                                                   // heads = z3^T gh
            const int tx = j - 32;
            step_gemm_41(a.z3 + r0 * kStepW + 64 * tx, kStepW, a.gh + r0 * kStepHeads, n, part + kStepWsOffHead + (int64_t)64 * tx * kStepHeads, lane);
        }
        return;
    }
    b -= dense_blocks;                                             // other_kernel = f_in^T gf: one contraction over max_other * rows rows
    const int64_t r0 = b * a.f_len;
    const int64_t n = (a.f_rows - r0 < a.f_len) ? a.f_rows - r0 : a.f_len;
    step_gemm_edge<kStepWsFilterIn>(a.f_in + r0 * kStepWsFilterIn, kStepWsFilterIn, a.gf + r0 * kStepH, kStepH, n,
                                    a.scratch + a.l1_slices * l1_partial + a.dense_slices * kStepWsDensePartial + b * kStepWsFilterPartial, kStepH, lane);
}

// one thread per float of the flat vector
__global__ __launch_bounds__(256) void step_ws_reduce_kernel(const StepWsReduceArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.total) return;
    int t = 0;
#pragma unroll
    for (int i = 1; i < kStepParams; ++i) t = e >= a.off[i] ? i : t;
    const int64_t k = e - a.off[t];
    if (k >= a.size[t]) { a.grads[e] = 0.0f; return; }             // padding between two variables
    const int A = a.num_actions;
    const float *dense = a.scratch + a.l1_slices * a.l1_partial;
    const float *src = nullptr;                                    // the entry in slice 0's partial; nullptr: a bias, `idx` into db
    int64_t stride = kStepWsDensePartial, count = a.dense_slices, idx = 0;
    switch (t) {
    case 0: src = dense + a.dense_slices * kStepWsDensePartial + k; stride = kStepWsFilterPartial; count = a.f_slices; break;
    case 1: idx = k; break;
    case 2: src = a.scratch + k; stride = a.l1_partial; count = a.l1_slices; break;
    case 3: idx = 256 + k; break;
    case 4: src = dense + kStepWsOffL2 + k; break;
    case 5: idx = 512 + k; break;
    case 6: src = dense + kStepWsOffFc1 + k; break;
    case 7: idx = 768 + k; break;
    case 8: src = dense + kStepWsOffHead + (k / A) * kStepHeads + (k % A); break;
    case 9: idx = 1024 + k; break;
    case 10: src = dense + kStepWsOffHead + k * kStepHeads + A; break;
    default: idx = 1024 + A; break;
    }
    float sum;
    if (src == nullptr) sum = a.db[idx];
    else {
        sum = src[0];
        for (int64_t s = 1; s < count; ++s) sum += src[s * stride];     // slice order, always
    }
    a.grads[e] = sum;
}

#endif  // CAVOID_POLICY_STEP_WS_KERNELS

}  // namespace cavoid
