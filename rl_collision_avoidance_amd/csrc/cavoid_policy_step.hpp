// cavoid_policy_step.hpp -- the rest of the trainer step behind cavoid_policy_weight_grads / cavoid_policy_apply (include/cavoid.h):
//   step_gemm_kernel     the five weight-gradient contractions X^T G of the LSTM network's trainer pass, cut into row slices: one
//                        wavefront forms one tile of one slice's partial product on v_mfma_f32_16x16x4_f32 (exact float32 products),
//                        straight from the pass's buffers;
//   step_reduce_kernel   sums every entry's partials in slice order and writes it into the flat gradient vector in the checkpoint's
//                        layout (the un-permutations of the packed LSTM / layer1 / head orders, db -> the six biases, zero padding);
//   step_norm_kernel     the twelve per-variable clip scales c / max(||g|| / n, c), one workgroup and one fixed-order reduction each;
//   step_apply_kernel    Adam or RMSProp on the float32 masters, one thread per entry of the flat vector.
// The partition into slices depends on the buffer rows and max_other only, and nothing here uses a floating-point atomic: the same
// buffers give the same bits.
//
// The tile of step_gemm.  For D = X^T G the MFMA's summation index is the ROW of the buffers: lane l holds A[i = l & 15][k = l >> 4] =
// X[row r + (l >> 4)][column of i] and B[k][j = l & 15] = G[row r + (l >> 4)][column of j].  Which column stands behind i is free, so a
// lane loads FOUR consecutive columns 4 i .. 4 i + 3 of its row with one 16-byte load and feeds them to four A tiles: tile ca holds the
// columns 4 i + ca of a 64-column block (and likewise cb for G).  One step of 4 rows is two 16-byte loads -- 256 contiguous bytes per
// row and operand -- and 16 MFMAs on a 64 x 64 tile; the result tile (ca, cb) holds D[4 i + ca][4 j + cb] at C/D position (i, j), i.e. a
// lane's four cb values of one register index are four consecutive output columns: one 16-byte store.
// The 72-wide operands (l1_in, h_in: 64 hidden, the host / input columns, padding) add an edge tile for columns 64..71 (one A tile, loaded
// one float per lane, columns 72..79 read as zero without touching memory), the 16-wide head gradient gh a tile with one B tile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cavoid.h"

namespace cavoid {

typedef float step_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kStepParams = 12;                  // CAVOID_POLICY_PARAMS
constexpr int kStepAlign = 64;                   // every variable of the flat vector starts on a multiple of this many floats
constexpr int kStepH = 64, kStepW = 256, kStepHost = 4, kStepOther = 7, kStepIn = 72, kStepHeads = 16;
constexpr int kStepBiasFloats = 1040;            // db: lstm 256 (packed gate order) | layer1 | layer2 | fullyconnected1 | heads 16
// the row slices of the contractions: a partial product per slice
constexpr int64_t kStepDenseSlice = 1024;        // rows of z / g per slice
constexpr int64_t kStepLstmSlice = 1024;         // rows of the flat [max_other * rows] LSTM operands per slice ...
constexpr int64_t kStepLstmSliceWide = 4096;     // ... once there are more than kStepLstmWideFrom of them
constexpr int64_t kStepLstmWideFrom = 4194304;
// one dense slice's partials: fullyconnected1 [256, 256] | layer2 [256, 256] | layer1 [72, 256] (packed rows) | heads [256, 16]
constexpr int64_t kStepOffFc1 = 0, kStepOffL2 = 65536, kStepOffL1 = 131072, kStepOffHead = kStepOffL1 + kStepIn * kStepW;
constexpr int64_t kStepDensePartial = kStepOffHead + kStepW * kStepHeads;
constexpr int64_t kStepLstmPartial = kStepIn * kStepW;          // [72, 256]: packed rows, packed gate columns
constexpr int kStepDenseJobs = 16 + 16 + 8 + 4, kStepLstmJobs = 8;

struct StepPartition { int64_t dense_slices, lstm_len, lstm_slices; };
__host__ __device__ inline StepPartition step_partition(int64_t rows, int32_t max_other) {
    StepPartition p;
    const int64_t t = rows * max_other;
    p.dense_slices = (rows + kStepDenseSlice - 1) / kStepDenseSlice;
    p.lstm_len = t > kStepLstmWideFrom ? kStepLstmSliceWide : kStepLstmSlice;
    p.lstm_slices = (t + p.lstm_len - 1) / p.lstm_len;
    return p;
}

// the flat parameter vector (cavoid_policy_param_layout)
struct StepLayout { int64_t off[kStepParams], size[kStepParams], total; };
inline StepLayout step_layout(int32_t num_actions) {
    const int64_t sizes[kStepParams] = {(kStepOther + kStepH) * 4 * kStepH, 4 * kStepH, (kStepHost + kStepH) * kStepW, kStepW, kStepW * kStepW, kStepW,
                                        kStepW * kStepW, kStepW, (int64_t)kStepW * num_actions, num_actions, kStepW, 1};
    StepLayout l;
    int64_t o = 0;
    for (int i = 0; i < kStepParams; ++i) {
        l.off[i] = o; l.size[i] = sizes[i]; l.total = o + sizes[i];
        o = (l.total + kStepAlign - 1) / kStepAlign * kStepAlign;
    }
    return l;
}

struct StepGemmArgs {
    const float *z1, *z2, *z3, *l1_in, *h_in, *gh, *g1, *g2, *g3, *gl;
    float *scratch;
    int64_t rows, lstm_rows;                     // buffer rows; max_other * buffer rows
    int64_t dense_slices, lstm_len, lstm_slices;
};

struct StepReduceArgs {
    const float *scratch, *db;
    float *grads;
    int64_t off[kStepParams], size[kStepParams], total;
    int64_t dense_slices, lstm_slices;
    int32_t num_actions;
};

struct StepApplyArgs {
    float *w[kStepParams];
    const float *grads, *clip_scale;             // clip_scale == nullptr: no clipping
    float *state1, *state2;
    int64_t *step;
    uint32_t *ticket;
    int64_t off[kStepParams], size[kStepParams], total;
    double lr, decay1, decay2, eps;
    int32_t kind;
};

struct StepNormArgs {
    const float *grads;
    float *clip_scale;
    int64_t off[kStepParams], size[kStepParams];
    double clip;
};

#if defined(CAVOID_POLICY_STEP_KERNELS) || defined(CAVOID_POLICY_STEP_TILES)
// the tiles: every translation unit with step GEMM jobs of its own instantiates them (cavoid_policy_step.hip, cavoid_policy_step_ws.hip)

#define STEP_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// 64 x 64 tile: x, g point at (first row of the slice, first column of the tile's 64-column block); n rows, a multiple of 4
__device__ __forceinline__ void step_gemm_44(const float *x, int ldx, const float *g, int ldg, int64_t n, float *out, int ldo, int lane) {
    step_f32x4 acc[4][4];
#pragma unroll
    for (int ca = 0; ca < 4; ++ca)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[ca][cb] = step_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int kq = lane >> 4, c4 = 4 * (lane & 15);
    const float *xp = x + (int64_t)kq * ldx + c4, *gp = g + (int64_t)kq * ldg + c4;
    // the loads of step r + 1 are issued in front of the 16 MFMAs of step r (the last one re-reads its own rows: no branch around a load)
    step_f32x4 a = *reinterpret_cast<const step_f32x4 *>(xp), b = *reinterpret_cast<const step_f32x4 *>(gp);
    for (int64_t r = 0; r < n; r += 4) {
        const int64_t rn = r + 4 < n ? r + 4 : r;
        const step_f32x4 an = *reinterpret_cast<const step_f32x4 *>(xp + rn * ldx);
        const step_f32x4 bn = *reinterpret_cast<const step_f32x4 *>(gp + rn * ldg);
#pragma unroll
        for (int ca = 0; ca < 4; ++ca)
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) acc[ca][cb] = STEP_MFMA(a[ca], b[cb], acc[ca][cb]);
        a = an; b = bn;
    }
#pragma unroll
    for (int ca = 0; ca < 4; ++ca)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * (4 * kq + r) + ca;
            *reinterpret_cast<step_f32x4 *>(out + (int64_t)row * ldo + c4) = step_f32x4{acc[ca][0][r], acc[ca][1][r], acc[ca][2][r], acc[ca][3][r]};
        }
}

// edge tile: LIVE (4 or 8) columns of x against a 64-column block of g -- the 72-wide operands' columns 64..71, the weight-sharing
// network's host columns 0..3 of l1_in and its 8-wide f_in.  x points at (first row, first live column), out at (first live row, the
// block's first column) of the partial.  The tile's columns LIVE..15 do not exist: zero, and never loaded (the address is clamped into
// the live ones)
template <int LIVE>
__device__ __forceinline__ void step_gemm_edge(const float *x, int ldx, const float *g, int ldg, int64_t n, float *out, int ldo, int lane) {
    static_assert(LIVE == 4 || LIVE == 8, "whole C/D row quads");
    step_f32x4 acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[cb] = step_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int kq = lane >> 4, i = lane & 15, c4 = 4 * i;
    const bool live = i < LIVE;
    const float *xp = x + (int64_t)kq * ldx + (i & (LIVE - 1)), *gp = g + (int64_t)kq * ldg + c4;
    float v = xp[0];
    step_f32x4 b = *reinterpret_cast<const step_f32x4 *>(gp);
    for (int64_t r = 0; r < n; r += 4) {
        const int64_t rn = r + 4 < n ? r + 4 : r;
        const float vn = xp[rn * ldx];
        const step_f32x4 bn = *reinterpret_cast<const step_f32x4 *>(gp + rn * ldg);
        const float a = live ? v : 0.0f;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[cb] = STEP_MFMA(a, b[cb], acc[cb]);
        v = vn; b = bn;
    }
    if (4 * kq < LIVE) {                                           // C/D rows 4 kq + r: the live ones
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *reinterpret_cast<step_f32x4 *>(out + (int64_t)(4 * kq + r) * ldo + c4) = step_f32x4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
    }
}

// a 64-column block of x against the 16-wide gh.  out points at the block's first row of the [256, 16] partial
__device__ __forceinline__ void step_gemm_41(const float *x, int ldx, const float *g, int64_t n, float *out, int lane) {
    step_f32x4 acc[4];
#pragma unroll
    for (int ca = 0; ca < 4; ++ca) acc[ca] = step_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int kq = lane >> 4, j = lane & 15;
    const float *xp = x + (int64_t)kq * ldx + 4 * j, *gp = g + (int64_t)kq * kStepHeads + j;
    step_f32x4 a = *reinterpret_cast<const step_f32x4 *>(xp);
    float b = gp[0];
    for (int64_t r = 0; r < n; r += 4) {
        const int64_t rn = r + 4 < n ? r + 4 : r;
        const step_f32x4 an = *reinterpret_cast<const step_f32x4 *>(xp + rn * ldx);
        const float bn = gp[rn * kStepHeads];
#pragma unroll
        for (int ca = 0; ca < 4; ++ca) acc[ca] = STEP_MFMA(a[ca], b, acc[ca]);
        a = an; b = bn;
    }
#pragma unroll
    for (int ca = 0; ca < 4; ++ca)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(int64_t)(4 * (4 * kq + r) + ca) * kStepHeads + j] = acc[ca][r];
}

#undef STEP_MFMA
#endif  // the tiles

#ifdef CAVOID_POLICY_STEP_KERNELS
// the kernels: cavoid_policy_step.hip alone (step_norm_kernel and step_apply_kernel take the layout as an argument: the weight-sharing
// network's step launches them through step_launch_update below)

// grid: dense_slices * kStepDenseJobs + lstm_slices * kStepLstmJobs workgroups of ONE wavefront
__global__ __launch_bounds__(64) void step_gemm_kernel(const StepGemmArgs a) {
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x, dense_blocks = a.dense_slices * kStepDenseJobs;
    if (b < dense_blocks) {
        const int64_t s = b / kStepDenseJobs, r0 = s * kStepDenseSlice;
        const int j = (int)(b % kStepDenseJobs);
        const int64_t n = (a.rows - r0 < kStepDenseSlice) ? a.rows - r0 : kStepDenseSlice;
        float *part = a.scratch + s * kStepDensePartial;
        if (j < 32) {                                              // fullyconnected1 = z2^T g3, layer2 = z1^T g2: 4 x 4 tiles each
            const float *x = (j < 16 ? a.z2 : a.z1) + r0 * kStepW, *g = (j < 16 ? a.g3 : a.g2) + r0 * kStepW;
            const int tx = (j & 15) >> 2, tg = j & 3;
            step_gemm_44(x + 64 * tx, kStepW, g + 64 * tg, kStepW, n, part + (j < 16 ? kStepOffFc1 : kStepOffL2) + (int64_t)64 * tx * kStepW + 64 * tg,
                         kStepW, lane);
        } else if (j < 36) {                                       // layer1 = l1_in^T g1, rows 0..63
            const int tg = j - 32;
            step_gemm_44(a.l1_in + r0 * kStepIn, kStepIn, a.g1 + r0 * kStepW + 64 * tg, kStepW, n, part + kStepOffL1 + 64 * tg, kStepW, lane);
        } else if (j < 40) {                                       // ... rows 64..71
            const int tg = j - 36;
            step_gemm_edge<kStepIn - 64>(a.l1_in + r0 * kStepIn + 64, kStepIn, a.g1 + r0 * kStepW + 64 * tg, kStepW, n,
                                         part + kStepOffL1 + 64 * kStepW + 64 * tg, kStepW, lane);
        } else {                                                   // heads = z3^T gh
            const int tx = j - 40;
            step_gemm_41(a.z3 + r0 * kStepW + 64 * tx, kStepW, a.gh + r0 * kStepHeads, n, part + kStepOffHead + (int64_t)64 * tx * kStepHeads, lane);
        }
    } else {                                                       // lstm = sum_t h_in[t]^T gl[t]: one contraction over max_other * rows rows
        const int64_t bl = b - dense_blocks, s = bl / kStepLstmJobs, r0 = s * a.lstm_len;
        const int j = (int)(bl % kStepLstmJobs), tg = j & 3;
        const int64_t n = (a.lstm_rows - r0 < a.lstm_len) ? a.lstm_rows - r0 : a.lstm_len;
        float *part = a.scratch + a.dense_slices * kStepDensePartial + s * kStepLstmPartial + 64 * tg;
        if (j < 4) step_gemm_44(a.h_in + r0 * kStepIn, kStepIn, a.gl + r0 * kStepW + 64 * tg, kStepW, n, part, kStepW, lane);
        else step_gemm_edge<kStepIn - 64>(a.h_in + r0 * kStepIn + 64, kStepIn, a.gl + r0 * kStepW + 64 * tg, kStepW, n, part + 64 * kStepW, kStepW, lane);
    }
}

// one thread per float of the flat vector
__global__ __launch_bounds__(256) void step_reduce_kernel(const StepReduceArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.total) return;
    int t = 0;
#pragma unroll
    for (int i = 1; i < kStepParams; ++i) t = e >= a.off[i] ? i : t;
    const int64_t k = e - a.off[t];
    if (k >= a.size[t]) { a.grads[e] = 0.0f; return; }             // padding between two variables
    const int A = a.num_actions;
    const float *src = nullptr;                                    // the entry in slice 0's partial; nullptr: a bias, `idx` into db
    int64_t stride = kStepDensePartial, count = a.dense_slices, idx = 0;
    const int c = (int)(k & (kStepW - 1)), d = (int)(k >> 8);      // (column, row) of a [*, 256] variable
    const int kc = 64 * ((c & 63) >> 4) + 16 * (c >> 6) + (c & 15);   // checkpoint gate column 64 gate + 16 w + u -> packed 64 w + 16 gate + u
    switch (t) {
    case 0: src = a.scratch + a.dense_slices * kStepDensePartial + (int64_t)(d < kStepOther ? kStepH + d : d - kStepOther) * kStepW + kc;
            stride = kStepLstmPartial; count = a.lstm_slices; break;
    case 1: idx = kc; break;
    case 2: src = a.scratch + kStepOffL1 + (int64_t)(d < kStepHost ? kStepH + d : d - kStepHost) * kStepW + c; break;
    case 3: idx = 256 + k; break;
    case 4: src = a.scratch + kStepOffL2 + k; break;
    case 5: idx = 512 + k; break;
    case 6: src = a.scratch + kStepOffFc1 + k; break;
    case 7: idx = 768 + k; break;
    case 8: src = a.scratch + kStepOffHead + (k / A) * kStepHeads + (k % A); break;
    case 9: idx = 1024 + k; break;
    case 10: src = a.scratch + kStepOffHead + k * kStepHeads + A; break;
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

// one workgroup per variable: the clip scale c / max(||g||_2 / n, c)
__global__ __launch_bounds__(1024) void step_norm_kernel(const StepNormArgs a) {
    __shared__ double part[1024];
    const int t = blockIdx.x, tid = threadIdx.x;
    const float *g = a.grads + a.off[t];
    const int64_t n = a.size[t];
    double s = 0.0;
    for (int64_t i = tid; i < n; i += 1024) { const double v = (double)g[i]; s += v * v; }
    part[tid] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const double avg = sqrt(part[0]) / (double)n;
        a.clip_scale[t] = (float)(a.clip / (avg > a.clip ? avg : a.clip));
    }
}

__device__ __forceinline__ double step_pow_int(double b, int64_t n) {
    double r = 1.0;
    while (n > 0) {
        if (n & 1) r *= b;
        b *= b;
        n >>= 1;
    }
    return r;
}

// one thread per float of the flat vector.  The element arithmetic is scalar float32, every operation rounded on its own (the build
// compiles with -ffp-contract=off); the coefficients are formed in double from the step count and rounded once.
__global__ __launch_bounds__(256) void step_apply_kernel(const StepApplyArgs a) {
    __shared__ int64_t step_before;
    if (threadIdx.x == 0) step_before = *a.step;
    __syncthreads();
    const int64_t t1 = step_before + 1;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < a.total) {
        int t = 0;
#pragma unroll
        for (int i = 1; i < kStepParams; ++i) t = e >= a.off[i] ? i : t;
        const int64_t k = e - a.off[t];
        if (k < a.size[t]) {                                       // (padding: nothing to update, the state stays what it is)
            float *wp = a.w[0];
#pragma unroll
            for (int i = 1; i < kStepParams; ++i) wp = t == i ? a.w[i] : wp;
            float g = a.grads[e];
            if (a.clip_scale != nullptr) g = g * a.clip_scale[t];
            const float w = wp[k];
            if (a.kind == 0) {                                     // CAVOID_OPT_ADAM
                const float b1 = (float)a.decay1, c1 = (float)(1.0 - a.decay1), b2 = (float)a.decay2, c2 = (float)(1.0 - a.decay2);
                const float step_size = (float)(a.lr / (1.0 - step_pow_int(a.decay1, t1)));
                const float root2 = (float)sqrt(1.0 - step_pow_int(a.decay2, t1));
                const float m = b1 * a.state1[e] + c1 * g;
                const float v = b2 * a.state2[e] + c2 * (g * g);
                const float denom = sqrtf(v) / root2 + (float)a.eps;
                a.state1[e] = m;
                a.state2[e] = v;
                wp[k] = w - step_size * (m / denom);
            } else {                                               // CAVOID_OPT_RMSPROP
                const float rho = (float)a.decay1, c1 = (float)(1.0 - a.decay1), mu = (float)a.decay2;
                const float ms = rho * a.state1[e] + c1 * (g * g);
                const float mom = mu * a.state2[e] + (float)a.lr * g / sqrtf(ms + (float)a.eps);
                a.state1[e] = ms;
                a.state2[e] = mom;
                wp[k] = w - mom;
            }
        }
    }
    // the step count: every workgroup has read it before it takes its ticket; the last one writes it (an ordinary store, one thread)
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const uint32_t ticket = atomicAdd(a.ticket, 1u);
        if (ticket == gridDim.x - 1) {
            *a.step = t1;
            *a.ticket = 0u;
        }
    }
}

#endif  // CAVOID_POLICY_STEP_KERNELS

// ---- host side, shared by cavoid_policy_step.hip and cavoid_policy_step_ws.hip ------------------------------------------------------
inline bool step_rows_ok(int64_t capacity_rows) { return capacity_rows > 0 && capacity_rows % 64 == 0 && capacity_rows / 64 <= 0x7fffffffLL; }
inline bool step_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool step_optimizer_ok(const cavoid_policy_optimizer *opt) {
    return opt && opt->struct_size == (int32_t)sizeof(cavoid_policy_optimizer) && (opt->kind == CAVOID_OPT_ADAM || opt->kind == CAVOID_OPT_RMSPROP) &&
           opt->state1 && opt->state2 && opt->step && opt->clip_average_norm >= 0.0;
}

}  // namespace cavoid

// step_norm_kernel (when clipping) and step_apply_kernel on the twelve masters in layout `l` (cavoid_policy_step.hip): the update of
// cavoid_policy_apply and cavoid_policy_apply_ws, up to the re-pack.  The caller has checked its arguments (step_optimizer_ok among them).
int cavoid_policy_step_update(cavoid_policy *h, float *const *masters, const cavoid::StepLayout &l, const cavoid_policy_optimizer *opt,
                              const float *grads_flat, hipStream_t stream);
