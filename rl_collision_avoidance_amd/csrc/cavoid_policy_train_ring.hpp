// cavoid_policy_train_ring.hpp -- the trainer's forward pass (forward + loss head + gradient at the heads) of NetworkVP_rnn for rows of
// 20..64 observed agents: the crowd step form's worlds (cavoid_crowd.hpp) observe up to 63 neighbours, policy_forward_kernel<4, true>
// (cavoid_policy.hpp) parks the whole padded input row in LDS and stops at kPolMaxOthers = 19 (80 + 16 + 8M + 8 <= 260).
//
// policy_train_ring_forward_kernel / policy_train_ring_regression_kernel are policy_forward_kernel<4, true> / policy_regression_forward_kernel<4>
// with the R = kPolMaxOthers input slots at LDS columns kPolXCol + 8 + 8s used as a RING (what SpRing is to the inference kernel,
// cavoid_policy_crowd.hpp):
//   * same workgroup (64 rows, 4 wavefronts), same LDS buffer (policy_lds_bytes(4), stride kPolStride, h / num_other / host columns), same
//     packed fragments and biases, policy_gemm, per-lane cell update (with its fence on keep / add), policy_heads<4, true, LOSS, false>;
//   * staging parks the host state and observed agents 0 .. min(M, R) - 1 -- the padded width stays 16 + 8 min(M, R) + 8 <= 176, inside
//     policy_div's range (the whole row, 536 at M = 64, is not); before LSTM step t slot t % R holds agent t;
//   * agent t + R (when a row of the tile runs step t + R) is loaded from global memory at the start of step t -- 64 rows x 7 values, at most
//     2 per thread, with their avg / std -- i.e. while step t's matrix instructions run, normalised by the staging's own expression
//     (v - avg) / std, and written into slot t % R behind the barrier that ends step t's GEMM; the step's second barrier publishes it, and
//     the slot's next readers are step t + R (its x_t) and step t + R - 1 (the upper half of its 16-wide input chunk: zero weights);
//   * step t's GEMM and its h_in[t] record read slot t % R.
// What they leave in memory is policy_forward_kernel<4, true>'s contract to the byte -- z1..z3, l1_in, h_in[t], the save records at
// (blockIdx.x * M + t), gh, loss[2], the heads' part of db -- so policy_backward_kernel<4> runs behind them unchanged: it walks
// t = M-1 .. 0 over those records in global memory and parks no input row.  Every index into save / h_in (and the backward's into gl) is
// formed in int64_t: at M = 64 and 2^25 rows the save index passes 2^31 records.
// On rows of <= R observed agents no slot is refilled before its last reader, and the kernels give bit for bit what the M <= 19 kernels
// give (tests/test_gpu_policy_train_ring.py).
//
// The kernels are policy_forward_tile<4, true, LOSS, PolRing<kPolTrainRing>> (cavoid_policy.hpp): the ring is that function's last template
// parameter, every ring statement sits behind `if constexpr (Ring::on)`, and the M <= 19 kernels compile to the instruction streams they had
// without it (profiles/policy_ring_fold_resources.txt).  This header keeps the ring's constants, its protocol and the two kernels.
#pragma once
#include "cavoid_policy.hpp"

namespace cavoid {

constexpr int kPolMaxOthersTrain = 64;          // the widest row the trainer pass takes (the env's own limit; ga3c/policy_kernel.py MAX_OTHERS_TRAIN)
constexpr int kPolTrainRing = kPolMaxOthers;    // R: every input slot the LDS row has -- the fewest refills

#ifdef CAVOID_POLICY_TRAIN_RING_KERNELS     /* compiled by cavoid_policy_train_ring.hip only */
__global__ void __launch_bounds__(256, 1) policy_train_ring_forward_kernel(const PolicyArgs p) {
    policy_forward_tile<4, true, kLossA3C, PolRing<kPolTrainRing>>(p);
}

// the supervised start's pass (cavoid_policy_train_regression on a crowd handle): the same forward with the regression head
__global__ void __launch_bounds__(256, 1) policy_train_ring_regression_kernel(const PolicyArgs p) {
    policy_forward_tile<4, true, kLossRegression, PolRing<kPolTrainRing>>(p);
}
#endif

}  // namespace cavoid
