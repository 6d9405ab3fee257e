// cavoid_policy_ws.hip -- C ABI (include/cavoid.h, cavoid_policy_*_ws) over the weight-sharing network's kernels of
// cavoid_policy_ws.hpp.  Own translation unit: the LSTM kernels of cavoid_policy_capi.hip are not rebuilt with them.
#include <hip/hip_runtime.h>

#include <new>

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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return CAVOID_ENODEVICE;
    HIP_TRY(hipSetDevice(device));
    cavoid_policy *h = new (std::nothrow) cavoid_policy();
    if (!h) return CAVOID_ENOMEM;
    h->device = device; h->max_other = max_other; h->num_actions = num_actions;
    h->in_size = 1 + kPolHost + kPolOther * max_other;
    h->ws = true; h->use_split = false;
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t o_frag = carve((size_t)ws_layout(max_other).end * sizeof(f32x4)), o_bias = carve(kBiasFloats * sizeof(float));
    const size_t o_avg = carve(h->in_size * sizeof(float)), o_std = carve(h->in_size * sizeof(float));
    const size_t o_step = carve(sizeof(int32_t)), o_done = carve(sizeof(uint32_t)), o_tick = carve(kPolCuSlots * sizeof(uint32_t));
    const size_t o_clamp = carve(sizeof(uint32_t));
    if (hipMalloc(&h->slab, off) != hipSuccess) { delete h; return CAVOID_ENOMEM; }
    if (hipMemset(h->slab, 0, off) != hipSuccess) { g_last_hip_error = (int)hipGetLastError(); (void)hipFree(h->slab); delete h; return CAVOID_EHIP; }
    unsigned char *b = static_cast<unsigned char *>(h->slab);
    h->frags = reinterpret_cast<f32x4 *>(b + o_frag); h->bias = reinterpret_cast<float *>(b + o_bias);
    h->avg = reinterpret_cast<float *>(b + o_avg); h->std = reinterpret_cast<float *>(b + o_std);
    h->step_counter = reinterpret_cast<int32_t *>(b + o_step); h->blocks_done = reinterpret_cast<uint32_t *>(b + o_done);
    h->cu_tickets = reinterpret_cast<uint32_t *>(b + o_tick);
    h->clamped_weights = reinterpret_cast<uint32_t *>(b + o_clamp);
    if (hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->num_cus <= 0) h->num_cus = 256;
    // 70 KB of LDS per 64-row workgroup, as the LSTM kernels: dynamic and opted into
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(policy_ws_forward_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)policy_lds_bytes(4)) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(policy_ws_forward_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)policy_lds_bytes(4)) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(policy_regression_ws_forward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)policy_lds_bytes(4)) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(policy_ws_backward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)policy_lds_bytes(4)) != hipSuccess) {
        g_last_hip_error = (int)hipGetLastError(); (void)hipFree(h->slab); delete h; return CAVOID_EHIP;
    }
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
    h->backward_loaded = w->with_backward != 0;
    h->normalize = w->avg != nullptr;
    if (h->normalize) {
        HIP_TRY(hipMemcpyAsync(h->avg, w->avg, h->in_size * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(h->std, w->std, h->in_size * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    h->min_policy = w->min_policy;
    h->loaded = true;
    return CAVOID_OK;
}

int cavoid_policy_ws_launch(cavoid_policy *h, const PolicyArgs &a, int64_t blocks, hipStream_t stream) {
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
    const int64_t rows64 = (rows + 63) / 64 * 64;
    if (b->capacity_rows < rows64 || b->capacity_rows % 64 != 0 || b->capacity_rows / 64 > 0x7fffffffLL || !b->z1 || !b->z2 || !b->z3 ||
        !b->l1_in || !b->f_in || !b->gh || !b->loss || !b->g1 || !b->g2 || !b->g3 || !b->gf || !b->db)
        return CAVOID_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemsetAsync(b->loss, 0, 2 * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(b->db, 0, kBiasFloats * sizeof(float), s));
    if (rows == 0) return CAVOID_OK;
    const int64_t cap = b->capacity_rows;
    PolicyWsArgs wa{};
    PolicyArgs &a = wa.a;
    a.x = x; a.rows = rows; a.stride = row_stride; a.max_other = h->max_other; a.num_actions = h->num_actions; a.in_size = h->in_size;
    a.avg = h->normalize ? h->avg : nullptr; a.std = h->normalize ? h->std : nullptr;
    a.frags = h->frags; a.bias = h->bias; a.min_policy = h->min_policy; a.cu_tickets = h->cu_tickets;
    a.y_r = y_r; a.a_idx = a_idx; a.beta = beta; a.log_eps = log_epsilon; a.rows64 = cap;
    a.z1 = b->z1; a.z2 = b->z2; a.z3 = b->z3; a.l1_in = b->l1_in; a.gh = b->gh; a.loss = b->loss; a.db = b->db;
    wa.f_in = b->f_in;
    // every tile of the buffers (tiles past `rows` carry zero gradients): the caller's GEMMs may run over all capacity_rows
    const unsigned blocks = (unsigned)(cap / 64);
    if (loss_kind == kLossRegression) hipLaunchKernelGGL(policy_regression_ws_forward_kernel, dim3(blocks), dim3(256), policy_lds_bytes(4), s, wa);
    else hipLaunchKernelGGL((policy_ws_forward_kernel<true>), dim3(blocks), dim3(256), policy_lds_bytes(4), s, wa);
    HIP_TRY(hipGetLastError());
    PolicyWsBackArgs k{};
    k.rows64 = cap; k.max_other = h->max_other; k.frags = h->frags;
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
