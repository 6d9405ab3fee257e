// cavoid_policy_wsring.hpp -- NetworkVP_rnn with MULTI_AGENT_ARCH 'weight_sharing' for rows of 20..64 observed neighbours: the actors'
// predict_p_and_v + select_action (policy_wsring_forward_kernel<false>) and the trainer's forward pass with either loss head
// (policy_wsring_forward_kernel<true>, policy_wsring_regression_kernel).  The crowd step form's worlds (cavoid_crowd.hpp) observe up to 63
// neighbours; policy_ws_forward_tile (cavoid_policy_ws.hpp) parks the whole padded input row in LDS and stops at kWsMaxOthers = 19
// (80 + 16 + 8M + 8 <= 260).
//
// The ring kernels are policy_ws_forward_tile<TRAIN, LOSS> with the R = kWsMaxOthers input slots at LDS columns kPolXCol + 8 + 8s used as
// a RING (what SpRing is to the LSTM inference kernel, cavoid_policy_crowd.hpp, and PolRing to its trainer pass,
// cavoid_policy_train_ring.hpp):
//   * same workgroup (64 rows, 4 wavefronts), same LDS buffer (policy_lds_bytes(4), stride kPolStride), same packed fragments and biases
//     (ws_layout(M) and policy_ws_pack_kernel hold for M <= 64: every fragment offset is int64_t, the largest k a pack thread forms is
//     16 * 1024 + 15), the filter MFMAs, policy_gemm per slot into the persistent layer1 accumulators, layer2 / fc1,
//     policy_heads<4, TRAIN, LOSS, false>, the row list, the action draw, policy_finish;
//   * staging parks the count, the host state and slots 0 .. min(M, R) - 1 -- the padded width stays 16 + 8 min(M, R) + 8 <= 176, inside
//     policy_div's range (the whole row, 536 at M = 64, is not); before slot i is processed ring slot i % R holds [xn_i (7) | is_on_i];
//   * slot i + R (when i + R < M) is loaded from global memory at the start of iteration i -- 64 rows x 8 values, two per thread, through
//     tile_row[] when a row list is given, with avg / std for the seven features -- normalised by the staging's own expression
//     (v - avg) / std, is_on by the staging's own comparison of the raw count (LDS column kPolXCol) with i + R + 1, and written into slot
//     i % R behind the loop's first barrier: by then every wavefront has read slot i.  The loop's second barrier publishes the write.
//     Tile rows at or past rows_here get zeros in all eight columns, as the staging leaves them;
//   * the last iteration's fifth K chunk (the host chunk at kPolXCol + 4) also reads ring slots 0 and 1, against zero weights: what is
//     parked there is finite as long as the input is.
// TRAIN leaves policy_ws_forward_kernel<true>'s memory contract to the byte -- l1_in [rows64, 4 + 64M], f_in[i] (copied from the ring slot
// during iteration i, not in one block at staging), z1..z3, gh, loss[2], the heads' part of db -- so policy_ws_backward_kernel runs behind
// it unchanged: it parks no input row, reads l1_in / z* / gh from global memory and forms every index that grows with M or the row count
// in int64_t (checked for M = 64 and 2^25 rows: row * w1, (i * rows64 + row) * 64 and i * kChWide * kFragPerChunkNarrow all are).
// On rows of <= R slots no ring slot is refilled before its last reader, and the kernels give bit for bit what the M <= 19 kernels give
// (tests/test_gpu_policy_wsring.py).
//
// The kernels are policy_ws_forward_tile<TRAIN, LOSS, PolRing<kWsRing>> (cavoid_policy_ws.hpp): the ring is that function's last template
// parameter, every ring statement sits behind `if constexpr (Ring::on)`, and the M <= 19 kernels compile to the instruction streams they had
// without it (profiles/policy_ring_fold_resources.txt).  This header keeps the ring's constants, its protocol and the three kernels.
//
// Not measured before this was written: at M = 64 the layer1 fragments are 257 chunks x 16 KB = 4.1 MB, past the "L2-resident" weight
// pack of M <= 19 (1.25 MB).  profiles/policy_wsring_timing.txt holds what that costs.
#pragma once
#include "cavoid_policy_ws.hpp"

namespace cavoid {

constexpr int kWsMaxOthersCrowd = 64;          // the widest weight-sharing row (the env's own limit; ga3c/policy_kernel.py MAX_OTHERS_WS_CROWD)
constexpr int kWsRing = kWsMaxOthers;          // R: every input slot the LDS row has -- the fewest refills

#ifdef CAVOID_POLICY_WSRING_KERNELS     /* compiled by cavoid_policy_wsring.hip only */
template <bool TRAIN>
__global__ void __launch_bounds__(256, TRAIN ? 1 : 2) policy_wsring_forward_kernel(const PolicyWsArgs wa) {
    policy_ws_forward_tile<TRAIN, kLossA3C, PolRing<kWsRing>>(wa);
}

// the supervised start's pass (cavoid_policy_train_regression_ws on a _create_ws_crowd handle): the same forward with the regression head
__global__ void __launch_bounds__(256, 1) policy_wsring_regression_kernel(const PolicyWsArgs wa) {
    policy_ws_forward_tile<true, kLossRegression, PolRing<kWsRing>>(wa);
}
#endif

}  // namespace cavoid
