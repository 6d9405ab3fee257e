// cavoid_policy_step.hip -- C ABI of the rest of the trainer step (include/cavoid.h: cavoid_policy_param_layout, _weight_grads_scratch,
// _weight_grads, _apply) over the kernels of cavoid_policy_step.hpp.  Own translation unit: no other kernel is rebuilt with these.
#include <hip/hip_runtime.h>

#include "cavoid.h"
#include "cavoid_host.hpp"
#define CAVOID_POLICY_STEP_KERNELS 1
#include "cavoid_policy_step.hpp"
#include "cavoid_policy_host.hpp"

using namespace cavoid;

static_assert(kStepParams == CAVOID_POLICY_PARAMS, "the header's count of variables");
static_assert(kStepBiasFloats == kBiasFloats && kStepIn == 72 && kStepHeads == 16, "the trainer pass's buffer widths");
static_assert(kStepDenseSlice % 64 == 0 && kStepLstmSlice % 64 == 0 && kStepLstmSliceWide % 64 == 0, "slices are whole 64-row tiles");

extern "C" int cavoid_policy_param_layout(int32_t max_other, int32_t num_actions, int64_t *offsets, int64_t *sizes, int64_t *total) {
    if (max_other < 1 || max_other > 64 || num_actions < 1 || num_actions > 15 || !offsets || !sizes || !total) return CAVOID_EINVAL;
    const StepLayout l = step_layout(num_actions);
    for (int i = 0; i < kStepParams; ++i) { offsets[i] = l.off[i]; sizes[i] = l.size[i]; }
    *total = l.total;
    return CAVOID_OK;
}

static int64_t step_scratch_floats(int64_t capacity_rows, int32_t max_other) {
    const StepPartition p = step_partition(capacity_rows, max_other);
    return p.dense_slices * kStepDensePartial + p.lstm_slices * kStepLstmPartial;
}

extern "C" int cavoid_policy_weight_grads_scratch(const cavoid_policy *h, int64_t capacity_rows, int64_t *floats) {
    if (!h || !floats) return CAVOID_EINVAL;
    if (h->ws) return CAVOID_EUNSUPPORTED;
    if (!step_rows_ok(capacity_rows)) return CAVOID_EINVAL;
    *floats = step_scratch_floats(capacity_rows, h->max_other);
    return CAVOID_OK;
}

extern "C" int cavoid_policy_weight_grads(cavoid_policy *h, const cavoid_policy_train_buffers *b, float *scratch, int64_t scratch_floats,
                                          float *grads_flat, void *stream) {
    if (!h) return CAVOID_EINVAL;
    if (h->ws) return CAVOID_EUNSUPPORTED;                 // (cavoid_policy_weight_grads_ws: other buffers, other jobs)
    if (!b || b->struct_size != (int32_t)sizeof(cavoid_policy_train_buffers) || !scratch || !grads_flat) return CAVOID_EINVAL;
    if (!step_rows_ok(b->capacity_rows)) return CAVOID_EINVAL;
    const float *const operands[] = {b->z1, b->z2, b->z3, b->l1_in, b->h_in, b->gh, b->g1, b->g2, b->g3, b->gl};
    for (const float *p : operands)
        if (!p || !step_aligned16(p)) return CAVOID_EINVAL;     // (the tiles are read with 16-byte loads)
    if (!b->db || !step_aligned16(scratch)) return CAVOID_EINVAL;
    if (scratch_floats < step_scratch_floats(b->capacity_rows, h->max_other)) return CAVOID_EINVAL;
    const StepPartition p = step_partition(b->capacity_rows, h->max_other);
    const int64_t blocks = p.dense_slices * kStepDenseJobs + p.lstm_slices * kStepLstmJobs;
    if (blocks > 0x7fffffffLL) return CAVOID_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(h->device));
    StepGemmArgs g{};
    g.z1 = b->z1; g.z2 = b->z2; g.z3 = b->z3; g.l1_in = b->l1_in; g.h_in = b->h_in; g.gh = b->gh; g.g1 = b->g1; g.g2 = b->g2; g.g3 = b->g3; g.gl = b->gl;
    g.scratch = scratch; g.rows = b->capacity_rows; g.lstm_rows = b->capacity_rows * h->max_other;
    g.dense_slices = p.dense_slices; g.lstm_len = p.lstm_len; g.lstm_slices = p.lstm_slices;
    hipLaunchKernelGGL(step_gemm_kernel, dim3((unsigned)blocks), dim3(64), 0, s, g);
    HIP_TRY(hipGetLastError());
    const StepLayout l = step_layout(h->num_actions);
    StepReduceArgs r{};
    r.scratch = scratch; r.db = b->db; r.grads = grads_flat; r.total = l.total;
    for (int i = 0; i < kStepParams; ++i) { r.off[i] = l.off[i]; r.size[i] = l.size[i]; }
    r.dense_slices = p.dense_slices; r.lstm_slices = p.lstm_slices; r.num_actions = h->num_actions;
    hipLaunchKernelGGL(step_reduce_kernel, dim3((unsigned)((l.total + 255) / 256)), dim3(256), 0, s, r);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

int cavoid_policy_step_update(cavoid_policy *h, float *const *masters, const StepLayout &l, const cavoid_policy_optimizer *opt, const float *grads_flat,
                              hipStream_t s) {
    const bool clip = opt->clip_average_norm > 0.0;
    if (clip) {
        StepNormArgs n{};
        n.grads = grads_flat; n.clip_scale = h->clip_scale; n.clip = opt->clip_average_norm;
        for (int i = 0; i < kStepParams; ++i) { n.off[i] = l.off[i]; n.size[i] = l.size[i]; }
        hipLaunchKernelGGL(step_norm_kernel, dim3(kStepParams), dim3(1024), 0, s, n);
        HIP_TRY(hipGetLastError());
    }
    StepApplyArgs a{};
    for (int i = 0; i < kStepParams; ++i) { a.w[i] = masters[i]; a.off[i] = l.off[i]; a.size[i] = l.size[i]; }
    a.grads = grads_flat; a.clip_scale = clip ? h->clip_scale : nullptr; a.state1 = opt->state1; a.state2 = opt->state2; a.step = opt->step;
    a.ticket = h->apply_ticket; a.total = l.total; a.lr = opt->lr; a.decay1 = opt->decay1; a.decay2 = opt->decay2; a.eps = opt->eps; a.kind = opt->kind;
    hipLaunchKernelGGL(step_apply_kernel, dim3((unsigned)((l.total + 255) / 256)), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

extern "C" int cavoid_policy_apply(cavoid_policy *h, const cavoid_policy_weights *w, const cavoid_policy_optimizer *opt, const float *grads_flat,
                                   void *stream) {
    if (!h) return CAVOID_EINVAL;
    if (h->ws) return CAVOID_EUNSUPPORTED;                 // (cavoid_policy_apply_ws: another layout, another pack)
    if (!w || w->struct_size != (int32_t)sizeof(cavoid_policy_weights) || !step_optimizer_ok(opt) || !grads_flat) return CAVOID_EINVAL;
    float *const masters[kStepParams] = {const_cast<float *>(w->lstm_kernel), const_cast<float *>(w->lstm_bias), const_cast<float *>(w->layer1_kernel),
                                         const_cast<float *>(w->layer1_bias), const_cast<float *>(w->layer2_kernel), const_cast<float *>(w->layer2_bias),
                                         const_cast<float *>(w->fc1_kernel), const_cast<float *>(w->fc1_bias), const_cast<float *>(w->p_kernel),
                                         const_cast<float *>(w->p_bias), const_cast<float *>(w->v_kernel), const_cast<float *>(w->v_bias)};
    for (const float *p : masters)
        if (!p) return CAVOID_EINVAL;
    if ((w->avg == nullptr) != (w->std == nullptr)) return CAVOID_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(h->device));
    if (const int rc = cavoid_policy_step_update(h, masters, step_layout(h->num_actions), opt, grads_flat, s)) return rc;
    return cavoid_policy_load(h, w, s);                    // the pack path itself: the handle is what a fresh load of the masters gives
}
