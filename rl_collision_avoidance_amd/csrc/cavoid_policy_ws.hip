// cavoid_policy_ws.hip -- C ABI (include/cavoid.h, cavoid_policy_*_ws) over the weight-sharing network's kernels of
// cavoid_policy_ws.hpp.  Own translation unit: the LSTM kernels of cavoid_policy_capi.hip are not rebuilt with them.
#include <hip/hip_runtime.h>

#include "cavoid.h"
#include "cavoid_host.hpp"
#define CAVOID_POLICY_WS_KERNELS 1
#include "cavoid_policy_ws.hpp"
#include "cavoid_policy_host.hpp"

using namespace cavoid;

extern "C" int cavoid_policy_create_ws(int32_t max_other, int32_t num_actions, int device, cavoid_policy **out) {
    if (!out) return CAVOID_EINVAL;
    *out = nullptr;
    if (max_other < 1 || max_other > kWsOthersRange || num_actions < 1 || num_actions > 15) return CAVOID_EINVAL;
    if (max_other > kWsMaxOthers) return CAVOID_EUNSUPPORTED;   // (the kernel parks the whole input row: 80 + 16 + 8M + 8 <= 260)
    cavoid_policy *h = nullptr;
    if (const int rc = policy_new_handle(max_other, num_actions, device, ws_layout(max_other).end, false, &h)) return rc;
    h->ws = true; h->use_split = false;
    const PolicyLdsOptIn kernels[] = {
        {reinterpret_cast<const void *>(policy_ws_forward_kernel<false>), policy_lds_bytes(4)},
        {reinterpret_cast<const void *>(policy_ws_forward_kernel<true>), policy_lds_bytes(4)},
        {reinterpret_cast<const void *>(policy_regression_ws_forward_kernel), policy_lds_bytes(4)},
        {reinterpret_cast<const void *>(policy_ws_backward_kernel), policy_lds_bytes(4)},
    };
    if (const int rc = policy_opt_in_lds(h, kernels)) return rc;
    *out = h;
    return CAVOID_OK;
}

extern "C" int cavoid_policy_load_ws(cavoid_policy *h, const cavoid_policy_weights *w, const float *other_kernel, const float *other_bias,
                                     void *stream) {
    if (!h || !w || w->struct_size != (int32_t)sizeof(cavoid_policy_weights) || !h->ws) return CAVOID_EINVAL;
    if (!other_kernel || !other_bias || !w->layer1_kernel || !w->layer1_bias || !w->layer2_kernel || !w->layer2_bias ||
        !w->fc1_kernel || !w->fc1_bias || !w->p_kernel || !w->p_bias || !w->v_kernel || !w->v_bias)
        return CAVOID_EINVAL;
    if ((w->avg == nullptr) != (w->std == nullptr)) return CAVOID_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(h->device));
    PolicyWsWeights k{};
    k.other_kernel = other_kernel; k.other_bias = other_bias; k.layer1_kernel = w->layer1_kernel; k.layer1_bias = w->layer1_bias;
    k.layer2_kernel = w->layer2_kernel; k.layer2_bias = w->layer2_bias; k.fc1_kernel = w->fc1_kernel; k.fc1_bias = w->fc1_bias;
    k.p_kernel = w->p_kernel; k.p_bias = w->p_bias; k.v_kernel = w->v_kernel; k.v_bias = w->v_bias;
    k.num_actions = h->num_actions; k.max_other = h->max_other;
    const WsLayout L = ws_layout(h->max_other);
    const int64_t n = w->with_backward ? L.end : L.fwd_end;
    const int64_t items = n > kBiasFloats ? n : kBiasFloats;
    hipLaunchKernelGGL(policy_ws_pack_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, k, h->frags, h->bias, n);
    HIP_TRY(hipGetLastError());
    return policy_finish_load(h, w, s);
}

int cavoid_policy_ws_backward_opt_in(cavoid_policy *h) {
    const PolicyLdsOptIn kernels[] = {{reinterpret_cast<const void *>(policy_ws_backward_kernel), policy_lds_bytes(4)}};
    return policy_opt_in_lds(h, kernels);
}

int cavoid_policy_ws_launch(cavoid_policy *h, const PolicyArgs &a, int64_t blocks, hipStream_t stream) {
    if (h->crowd) return cavoid_policy_wsring_launch(h, a, blocks, stream);    // (20..64 slots: the input slots as a ring)
    const PolicyWsArgs wa{a, nullptr};
    hipLaunchKernelGGL((policy_ws_forward_kernel<false>), dim3((unsigned)blocks), dim3(256), policy_lds_bytes(4), stream, wa);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

// the trainer pass with either loss head (kLossA3C: cavoid_policy_train_ws; kLossRegression: cavoid_policy_train_regression_ws)
static int policy_train_ws(cavoid_policy *h, const float *x, int64_t rows, int64_t row_stride, const float *y_r, const int32_t *a_idx,
                           float beta, float log_epsilon, const cavoid_policy_train_ws_buffers *b, void *stream, int loss_kind) {
    if (!h || !x || !y_r || !a_idx || !b || b->struct_size != (int32_t)sizeof(cavoid_policy_train_ws_buffers) || !h->ws) return CAVOID_EINVAL;
    if (!h->loaded || !h->backward_loaded || rows < 0 || row_stride < h->in_size) return CAVOID_EINVAL;
    if (!b->f_in || !b->gf) return CAVOID_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    PolicyWsArgs wa{};
    unsigned blocks = 0;
    if (const int rc = policy_train_begin(h, x, rows, row_stride, y_r, a_idx, beta, log_epsilon, b, s, &wa.a, &blocks)) return rc;
    if (blocks == 0) return CAVOID_OK;
    wa.f_in = b->f_in;
    if (h->crowd) {                                        // (the forward parks R slots of the row at a time: cavoid_policy_wsring.hpp)
        if (const int rc = cavoid_policy_wsring_train_launch(h, wa.a, wa.f_in, blocks, loss_kind, s)) return rc;
    } else if (loss_kind == kLossRegression) hipLaunchKernelGGL(policy_regression_ws_forward_kernel, dim3(blocks), dim3(256), policy_lds_bytes(4), s, wa);
    else hipLaunchKernelGGL((policy_ws_forward_kernel<true>), dim3(blocks), dim3(256), policy_lds_bytes(4), s, wa);
    HIP_TRY(hipGetLastError());
    PolicyWsBackArgs k{};
    k.rows64 = wa.a.rows64; k.max_other = h->max_other; k.frags = h->frags;
    k.z1 = b->z1; k.z2 = b->z2; k.z3 = b->z3; k.gh = b->gh; k.l1_in = b->l1_in; k.g1 = b->g1; k.g2 = b->g2; k.g3 = b->g3; k.gf = b->gf; k.db = b->db;
    hipLaunchKernelGGL(policy_ws_backward_kernel, dim3(blocks), dim3(256), policy_lds_bytes(4), s, k);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

extern "C" int cavoid_policy_train_ws(cavoid_policy *h, const float *x, int64_t rows, int64_t row_stride, const float *y_r,
                                      const int32_t *a_idx, float beta, float log_epsilon, const cavoid_policy_train_ws_buffers *b,
                                      void *stream) {
    return policy_train_ws(h, x, rows, row_stride, y_r, a_idx, beta, log_epsilon, b, stream, kLossA3C);
}

extern "C" int cavoid_policy_train_regression_ws(cavoid_policy *h, const float *x, int64_t rows, int64_t row_stride, const float *y_r,
                                                 const int32_t *a_idx, const cavoid_policy_train_ws_buffers *b, void *stream) {
    return policy_train_ws(h, x, rows, row_stride, y_r, a_idx, 0.0f, 0.0f, b, stream, kLossRegression);
}
