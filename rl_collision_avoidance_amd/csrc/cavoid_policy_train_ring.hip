// cavoid_policy_train_ring.hip -- the trainer's forward pass on a crowd handle (20..64 observed agents): the ring kernels of
// cavoid_policy_train_ring.hpp behind cavoid_policy_train / cavoid_policy_train_regression (cavoid_policy_capi.hip).  Own translation
// unit: the kernels of cavoid_policy_capi.hip are not rebuilt with them.
#include <hip/hip_runtime.h>

#include "cavoid.h"
#include "cavoid_host.hpp"
#define CAVOID_POLICY_TRAIN_RING_KERNELS 1
#include "cavoid_policy_train_ring.hpp"
#include "cavoid_policy_host.hpp"

using namespace cavoid;

static_assert(kPolXCol + 8 + 8 * kPolTrainRing + 16 <= kPolStride, "the ring's slots and the zero columns behind the last one fit the LDS row");
static_assert(16 + 8 * kPolTrainRing + 8 <= 512, "the staged width stays inside policy_div's range");

int cavoid_policy_train_ring_opt_in(cavoid_policy *h) {
    const PolicyLdsOptIn kernels[] = {
        {reinterpret_cast<const void *>(policy_train_ring_forward_kernel), policy_lds_bytes(4)},
        {reinterpret_cast<const void *>(policy_train_ring_regression_kernel), policy_lds_bytes(4)},
    };
    return policy_opt_in_lds(h, kernels);
}

int cavoid_policy_train_ring_launch(cavoid_policy *h, const PolicyArgs &a, unsigned blocks, int loss_kind, hipStream_t stream) {
    if (!h->crowd || h->max_other > kPolMaxOthersTrain) return CAVOID_EUNSUPPORTED;
    if (loss_kind == kLossRegression) hipLaunchKernelGGL(policy_train_ring_regression_kernel, dim3(blocks), dim3(256), policy_lds_bytes(4), stream, a);
    else hipLaunchKernelGGL(policy_train_ring_forward_kernel, dim3(blocks), dim3(256), policy_lds_bytes(4), stream, a);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}
