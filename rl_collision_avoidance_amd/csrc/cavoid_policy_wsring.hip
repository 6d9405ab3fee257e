// cavoid_policy_wsring.hip -- the weight-sharing network on rows of 20..64 observed neighbours: cavoid_policy_create_ws_crowd and the
// ring kernels of cavoid_policy_wsring.hpp behind cavoid_policy_forward / _forward_rows / _train_ws / _train_regression_ws
// (cavoid_policy_ws.hip routes a handle with ws and crowd both set here).  Own translation unit: the kernels of cavoid_policy_ws.hip are
// not rebuilt with them.
#include <hip/hip_runtime.h>

#include "cavoid.h"
#include "cavoid_host.hpp"
#define CAVOID_POLICY_WSRING_KERNELS 1
#include "cavoid_policy_wsring.hpp"
#include "cavoid_policy_host.hpp"

using namespace cavoid;

static_assert(kPolXCol + 8 + 8 * kWsRing + 16 <= kPolStride, "the ring's slots and the zero columns behind the last one fit the LDS row");
static_assert(16 + 8 * kWsRing + 8 <= 512, "the staged width stays inside policy_div's range");
static_assert(kWsMaxOthersCrowd <= kWsOthersRange, "the env's own limit");

extern "C" int cavoid_policy_create_ws_crowd(int32_t max_other, int32_t num_actions, int device, cavoid_policy **out) {
    if (!out) return CAVOID_EINVAL;
    *out = nullptr;
    if (max_other < 1 || max_other > kWsMaxOthersCrowd || num_actions < 1 || num_actions > 15) return CAVOID_EINVAL;
    if (max_other <= kWsMaxOthers) return CAVOID_EUNSUPPORTED;   // (cavoid_policy_create_ws: the kernels that park the whole row)
    cavoid_policy *h = nullptr;
    if (const int rc = policy_new_handle(max_other, num_actions, device, ws_layout(max_other).end, false, &h)) return rc;
    h->ws = true; h->crowd = true; h->use_split = false;
    const PolicyLdsOptIn kernels[] = {
        {reinterpret_cast<const void *>(policy_wsring_forward_kernel<false>), policy_lds_bytes(4)},
        {reinterpret_cast<const void *>(policy_wsring_forward_kernel<true>), policy_lds_bytes(4)},
        {reinterpret_cast<const void *>(policy_wsring_regression_kernel), policy_lds_bytes(4)},
    };
    if (const int rc = policy_opt_in_lds(h, kernels)) return rc;
    if (const int rc = cavoid_policy_ws_backward_opt_in(h)) return rc;
    *out = h;
    return CAVOID_OK;
}

int cavoid_policy_wsring_launch(cavoid_policy *h, const PolicyArgs &a, int64_t blocks, hipStream_t stream) {
    if (!h->ws || !h->crowd || h->max_other > kWsMaxOthersCrowd) return CAVOID_EUNSUPPORTED;
    const PolicyWsArgs wa{a, nullptr};
    hipLaunchKernelGGL((policy_wsring_forward_kernel<false>), dim3((unsigned)blocks), dim3(256), policy_lds_bytes(4), stream, wa);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

int cavoid_policy_wsring_train_launch(cavoid_policy *h, const PolicyArgs &a, float *f_in, unsigned blocks, int loss_kind, hipStream_t stream) {
    if (!h->ws || !h->crowd || h->max_other > kWsMaxOthersCrowd) return CAVOID_EUNSUPPORTED;
    const PolicyWsArgs wa{a, f_in};
    if (loss_kind == kLossRegression) hipLaunchKernelGGL(policy_wsring_regression_kernel, dim3(blocks), dim3(256), policy_lds_bytes(4), stream, wa);
    else hipLaunchKernelGGL((policy_wsring_forward_kernel<true>), dim3(blocks), dim3(256), policy_lds_bytes(4), stream, wa);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}
