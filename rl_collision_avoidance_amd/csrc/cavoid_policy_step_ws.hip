// cavoid_policy_step_ws.hip -- C ABI of the rest of the trainer step for the weight-sharing network (include/cavoid.h:
// cavoid_policy_param_layout_ws, _weight_grads_scratch_ws, _weight_grads_ws, _apply_ws) over the kernels of cavoid_policy_step_ws.hpp and the
// update launches of cavoid_policy_step.hip.  Own translation unit: no other kernel is rebuilt with these.
#include <hip/hip_runtime.h>

#include "cavoid.h"
#include "cavoid_host.hpp"
#define CAVOID_POLICY_STEP_TILES 1
#define CAVOID_POLICY_STEP_WS_KERNELS 1
#include "cavoid_policy_step_ws.hpp"
#include "cavoid_policy_host.hpp"

using namespace cavoid;

static_assert(kStepBiasFloats == kBiasFloats && kStepWsFilterIn == 8 && kStepHeads == 16, "the trainer pass's buffer widths");
static_assert(kStepDenseSlice % 64 == 0 && kStepWsL1Slice % 64 == 0 && kStepWsFilterSlice % 64 == 0 && kStepWsFilterSliceWide % 64 == 0,
              "slices are whole 64-row tiles");

extern "C" int cavoid_policy_param_layout_ws(int32_t max_other, int32_t num_actions, int64_t *offsets, int64_t *sizes, int64_t *total) {
    if (max_other < 1 || max_other > 64 || num_actions < 1 || num_actions > 15 || !offsets || !sizes || !total) return CAVOID_EINVAL;
    const StepLayout l = step_ws_layout(max_other, num_actions);
    for (int i = 0; i < kStepParams; ++i) { offsets[i] = l.off[i]; sizes[i] = l.size[i]; }
    *total = l.total;
    return CAVOID_OK;
}

extern "C" int cavoid_policy_weight_grads_scratch_ws(const cavoid_policy *h, int64_t capacity_rows, int64_t *floats) {
    if (!h || !floats) return CAVOID_EINVAL;
    if (!h->ws) return CAVOID_EUNSUPPORTED;
    if (!step_rows_ok(capacity_rows)) return CAVOID_EINVAL;
    *floats = step_ws_scratch_floats(capacity_rows, h->max_other);
    return CAVOID_OK;
}

extern "C" int cavoid_policy_weight_grads_ws(cavoid_policy *h, const cavoid_policy_train_ws_buffers *b, float *scratch, int64_t scratch_floats,
                                             float *grads_flat, void *stream) {
    if (!h) return CAVOID_EINVAL;
    if (!h->ws) return CAVOID_EUNSUPPORTED;                // (cavoid_policy_weight_grads: the LSTM network's buffers and jobs)
    if (!b || b->struct_size != (int32_t)sizeof(cavoid_policy_train_ws_buffers) || !scratch || !grads_flat) return CAVOID_EINVAL;
    if (!step_rows_ok(b->capacity_rows)) return CAVOID_EINVAL;
    const float *const operands[] = {b->z1, b->z2, b->z3, b->l1_in, b->f_in, b->gh, b->g1, b->g2, b->g3, b->gf};
    for (const float *p : operands)
        if (!p || !step_aligned16(p)) return CAVOID_EINVAL;     // (the tiles are read with 16-byte loads)
    if (!b->db || !step_aligned16(scratch)) return CAVOID_EINVAL;
    if (scratch_floats < step_ws_scratch_floats(b->capacity_rows, h->max_other)) return CAVOID_EINVAL;
    const StepWsPartition p = step_ws_partition(b->capacity_rows, h->max_other);
    const int64_t blocks = p.l1_slices * 4 * (h->max_other + 1) + p.dense_slices * kStepWsDenseJobs + p.f_slices;
    if (blocks > 0x7fffffffLL) return CAVOID_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(h->device));
    StepWsGemmArgs g{};
    g.z1 = b->z1; g.z2 = b->z2; g.z3 = b->z3; g.l1_in = b->l1_in; g.f_in = b->f_in; g.gh = b->gh; g.g1 = b->g1; g.g2 = b->g2; g.g3 = b->g3; g.gf = b->gf;
    g.scratch = scratch; g.rows = b->capacity_rows; g.f_rows = b->capacity_rows * h->max_other;
    g.dense_slices = p.dense_slices; g.l1_len = p.l1_len; g.l1_slices = p.l1_slices; g.f_len = p.f_len; g.f_slices = p.f_slices;
    g.max_other = h->max_other;
    hipLaunchKernelGGL(step_ws_gemm_kernel, dim3((unsigned)blocks), dim3(64), 0, s, g);
    HIP_TRY(hipGetLastError());
    const StepLayout l = step_ws_layout(h->max_other, h->num_actions);
    StepWsReduceArgs r{};
    r.scratch = scratch; r.db = b->db; r.grads = grads_flat; r.total = l.total;
    for (int i = 0; i < kStepParams; ++i) { r.off[i] = l.off[i]; r.size[i] = l.size[i]; }
    r.dense_slices = p.dense_slices; r.l1_slices = p.l1_slices; r.f_slices = p.f_slices; r.l1_partial = step_ws_l1_partial(h->max_other);
    r.num_actions = h->num_actions;
    hipLaunchKernelGGL(step_ws_reduce_kernel, dim3((unsigned)((l.total + 255) / 256)), dim3(256), 0, s, r);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

extern "C" int cavoid_policy_apply_ws(cavoid_policy *h, const cavoid_policy_weights *w, const float *other_kernel, const float *other_bias,
                                      const cavoid_policy_optimizer *opt, const float *grads_flat, void *stream) {
    if (!h) return CAVOID_EINVAL;
    if (!h->ws) return CAVOID_EUNSUPPORTED;
    if (!w || w->struct_size != (int32_t)sizeof(cavoid_policy_weights) || !step_optimizer_ok(opt) || !grads_flat) return CAVOID_EINVAL;
    float *const masters[kStepParams] = {const_cast<float *>(other_kernel), const_cast<float *>(other_bias), const_cast<float *>(w->layer1_kernel),
                                         const_cast<float *>(w->layer1_bias), const_cast<float *>(w->layer2_kernel), const_cast<float *>(w->layer2_bias),
                                         const_cast<float *>(w->fc1_kernel), const_cast<float *>(w->fc1_bias), const_cast<float *>(w->p_kernel),
                                         const_cast<float *>(w->p_bias), const_cast<float *>(w->v_kernel), const_cast<float *>(w->v_bias)};
    for (const float *p : masters)
        if (!p) return CAVOID_EINVAL;
    if ((w->avg == nullptr) != (w->std == nullptr)) return CAVOID_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(h->device));
    if (const int rc = cavoid_policy_step_update(h, masters, step_ws_layout(h->max_other, h->num_actions), opt, grads_flat, s)) return rc;
    return cavoid_policy_load_ws(h, w, other_kernel, other_bias, s);   // the pack path itself: the handle is what a fresh load of the masters gives
}
