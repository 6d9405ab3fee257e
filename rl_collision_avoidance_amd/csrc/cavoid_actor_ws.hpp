// cavoid_actor_ws.hpp -- actor_ws_kernel<N, RVO>: the closed actor loop of cavoid_actor.hpp (K env steps in ONE launch) for the
// weight-sharing network (MULTI_AGENT_ARCH 'weight_sharing', cavoid_policy_ws.hpp) -- cavoid_actor_run_ws.
//
// actor_kernel's step loop with the weight-sharing pass as its policy phase.  Per tile of floor(64/N) worlds x N agents (up to 64
// policy rows) one workgroup of four wavefronts runs, K times:
//
//   all 4 wavefronts   policy_ws_forward_tile (FUSED): the whole float32-MFMA pass of the tile's rows that need an action, read in
//                      place from the observation the env wrote, + the Philox action draw -> actions / values of the tile
//   wavefront 0        env.step of the tile + the Experience bookkeeping of its slots (actor_env_push_tile), LDS carved out of the
//   wavefronts 1..3    pass's activation rows, which are idle now; meanwhile the step's state rows -> the experience ring
//                      (rollout_copy_rows) -- or all four wavefronts on the cooperative env step (actor_env_push_tile_quad)
//
// LDS (policy_lds_bytes(4) = 71 008 B, two workgroups per CU):
//   [0, 66 560)        the activation rows [64][kPolStride] -- LENT to the env step between two passes (the split form of actor_kernel
//                      lends 2 * kSpPlaneB = 67 584 B: the host's fit check is this kernel's own, actor_ws_lent_bytes())
//   [66 560, 70 720)   the packed biases (rewritten by every pass)
//   [70 720, 70 752)   8 ints: [4] the CU ticket, [6], [7] the mask of the rows that need an action at the next step (live_next of the
//                      tile's own env step) -- behind the lent region, so that the env step's scratch cannot reach it
//   [70 752, 71 008)   the pass's row list
//
// Rows that need no action (a finished agent waiting for its world's last learning agent, a scripted agent, an absent slot) do not go
// through the network: the live rows are handed to the pass as its row list (a row's results do not depend on its place in the tile and
// the action draw is keyed by the global row and the step), the others get action 0 / value 0 -- what the step-by-step path's row-list
// pass (cavoid_rollout_active_rows + cavoid_policy_forward_rows) leaves.  With the re-flush quirk every row counts.  Every value is
// computed by the statements of the step-by-step path in the same order: trajectories, experience rings and episode logs are
// bit-identical to it (tests/test_gpu_actor_ws.py).
#pragma once
#include "cavoid_actor.hpp"
#include "cavoid_policy_ws.hpp"

namespace cavoid {

// what the pass lends the env step: its activation rows
__host__ __device__ constexpr size_t actor_ws_lent_bytes() { return (size_t)64 * kPolStride * sizeof(float); }
static_assert(actor_ws_lent_bytes() + (kBiasFloats + 8 + 64) * sizeof(float) == policy_lds_bytes(4), "the LDS map above");

template <int N, bool RVO>
__global__ void __launch_bounds__(256, 2) actor_ws_kernel(const KCfg c, const KState s, const PoolRec *pool, const PolicyWsArgs wa_arg, const RolloutCfg rc,
                                                          const RolloutState rs, const RolloutIO rio_arg, const ActorIO io) {
    extern __shared__ __attribute__((aligned(16))) float act[];                  // the pass's activation rows ...
    int *ticket_slot = ws_ticket_slot(act);
    int &ticket = ticket_slot[4];
    int *live_next = ticket_slot + 6;
    int *tile_row = ws_tile_row(act);
    double *lds_tab = reinterpret_cast<double *>(act);                           // ... lent to the env step while they are idle
    float *wbase = act + lds_floats_block();

    const PolicyArgs &p = wa_arg.a;
    const int tid0 = threadIdx.x;
    const int wpw = c.wpw, ow = c.width;
    const int64_t tile = blockIdx.x, w0 = tile * wpw, a0 = w0 * N;
    int64_t worlds_here = c.num_worlds - w0;
    worlds_here = worlds_here > wpw ? wpw : (worlds_here < 0 ? 0 : worlds_here);
    const int rows = (int)worlds_here * N;                   // policy rows = agent slots of this tile
    const int32_t step0 = *io.rollout_step, pstep0 = *p.step_counter;

    if (tid0 == 0) ticket = policy_cu_ticket(p.cu_tickets);   // arrival parity on the CU -> static priority (policy_cu_ticket, cavoid_policy.hpp)
    __syncthreads();
    if (ticket & 1) __builtin_amdgcn_s_setprio(1);

#pragma unroll 1
    for (int t = 0; t < io.n_steps; ++t) {
        // (re-materialised per step: everything derived from the thread id is loop invariant and would be hoisted out of the step loop
        //  into registers live across the whole body -- cavoid_actor.hpp)
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const int wave_in_block = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        const float *obs_t = io.obs[t & 1];
        float *obs_n = io.obs[(t + 1) & 1];
        const int32_t step = step0 + t;
        const int blk = step % rc.ring_len;

        // ---- predict_p_and_v + select_action for the tile's rows that need an action -----------------------------------------------
        {
            // the predicate of actor_kernel (cavoid_rollout_active_rows' on the step-by-step path): obs column 0 set, and the agent not done
            // in the step that produced this observation unless its world has just restarted
            bool mine = lane < rows;
            if (rc.reflush_done == 0) {
                if (t == 0) {                                // (uniform) from the WORLD STATE: a learning agent whose state carries no terminal flag
                    if (mine) mine = obs_t[(a0 + lane) * ow] > 0.5f && (s.flags[a0 + lane] & CAVOID_F_DONE_MASK) == 0u;
                } else {                                     // the later ones: the mask the tile's own env step left in LDS
                    const unsigned long long m = (unsigned long long)(uint32_t)live_next[0] | ((unsigned long long)(uint32_t)live_next[1] << 32);
                    mine = (m >> lane) & 1ull;
                }
            }
            // (a row that needs no action is handed action 0 / value 0, what the step-by-step path's row-list pass leaves there)
            if (wave_in_block == 0 && lane < rows && !mine) { io.actions[a0 + lane] = 0; io.values[a0 + lane] = 0.0f; }
            const unsigned long long live_mask = __ballot(mine);            // (every wavefront evaluates the same 64 rows: no trip through LDS)
            const int n_live = __popcll(live_mask);
            if (n_live > 0) {                                // (uniform over the workgroup; 0: nobody in the tile needs an action)
                // the live rows, in order, as the pass's row list (global rows: it gathers them from p.x and scatters the outputs)
                if (wave_in_block == 0 && mine) tile_row[__popcll(live_mask & ((1ull << lane) - 1ull))] = (int)(a0 + lane);
                __syncthreads();
                PolicyWsArgs wa = wa_arg;
                wa.a.x = obs_t + 1;                          // column 0 (is_learning) is not a network input
                wa.a.v_out = io.values; wa.a.actions_out = io.actions; wa.a.greedy = io.greedy;
                policy_ws_forward_tile<false, kLossA3C, PolNoRing, true>(wa, tid, n_live, pstep0 + t);
            }
        }
        __syncthreads();                                     // the tile's actions / values are in memory; the activation rows are idle

        if (!RVO && N <= kActorQuadMaxAgents && io.quad) {   // (uniform)
            // ---- the step's state rows -> the experience store by wavefronts 1..3, then env.step of the tile by all four (cavoid_quad.hpp)
            //      and the Experience bookkeeping of its slots by wavefront 0
            if (wave_in_block != 0) rollout_copy_rows(rc, obs_t, rio_arg.x, a0, rows, blk, tid - 64, 192);
            actor_env_push_tile_quad<(N <= kActorQuadMaxAgents ? N : 1), true>(c, s, pool, rc, rs, rio_arg, io, obs_t, obs_n, reinterpret_cast<unsigned char *>(act),
                                                                              wave_in_block, lane, tile, step, blk, live_next);
        } else if (wave_in_block == 0) {
            // ---- env.step of the tile, then the Experience bookkeeping of its slots ---------------------------------------
            actor_env_push_tile<N, RVO, (N <= (RVO ? 9 : 13))>(c, s, pool, rc, rs, rio_arg, io, obs_t, obs_n, lds_tab, wbase, lane, tile, step, blk, live_next);
        } else {
            // ---- meanwhile: the step's state rows -> the time-major experience store -----------------------------------------
            rollout_copy_rows(rc, obs_t, rio_arg.x, a0, rows, blk, tid - 64, 192);
        }
        __syncthreads();                                     // obs(t+1), the world state, the slot state and live_next are in place
    }
}

}  // namespace cavoid
