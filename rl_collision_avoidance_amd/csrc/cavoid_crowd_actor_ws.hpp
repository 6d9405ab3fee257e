// cavoid_crowd_actor_ws.hpp -- crowd_ws_rollout_kernel<NB, RVO>: the closed actor loop of crowd worlds (17..64 agents, cavoid_crowd.hpp) for the
// weight-sharing network (MULTI_AGENT_ARCH 'weight_sharing'), K env steps in ONE launch -- cavoid_crowd_actor_run_ws.
//
// crowd_actor_kernel's launch shape (cavoid_crowd_actor.hpp) with actor_ws_kernel's policy phase (cavoid_actor_ws.hpp).  A crowd tile is
// floor(64/n) worlds x n agents <= 64 rows: one 64-row policy tile.  One workgroup of four wavefronts per tile runs, per step:
//
//   all 4 wavefronts   policy_ws_forward_tile<false, kLossA3C, PolRing<kWsRing>, true>: the float32-MFMA weight-sharing pass of the tile's rows
//                      that need an action -- compacted into the pass's row list -- with the R = 19 input slots as a ring (rows of up to 63
//                      observed neighbours), + the Philox action draw -> actions / values of the tile
//   wavefront 0        env.step of the tile (crowd_tile<NB, MODE_STEP_AUTORESET_N, RVO>, one step) and the Experience bookkeeping of its slots
//   wavefronts 1..3    meanwhile: the step's state rows -> the time-major experience ring (rollout_copy_rows)
//                      -- crowd_actor_env_phase, the statements crowd_actor_kernel runs
//
// LDS (policy_lds_bytes(4) = 71 008 B, two workgroups per CU) is actor_ws_kernel's map:
//   [0, 66 560)        the activation rows [64][kPolStride] -- LENT to the env step between two passes: the action table at 0, the wavefront's
//                      arrays behind it (crowd_kernel's allocation, at most 64 KB; the host checks crowd_actor_env_lds_bytes against both)
//   [66 560, 70 720)   the packed biases (rewritten by every pass)
//   [70 720, 70 752)   8 ints: [4] the CU ticket, [6], [7] the mask of the rows that need an action at the next step -- behind the lent region
//   [70 752, 71 008)   the pass's row list
//
// ONE ring instantiation serves every neighbour count: with M <= R no slot is refilled and the ring statements compute what the whole-row
// kernel computes (cavoid_policy_wsring.hpp), and a cavoid_policy_create_ws handle (M <= 19) and a _create_ws_crowd handle (20..64) share
// ws_layout(M).  Unlike crowd_actor_kernel's ring pass this one IS compacted: rows that need no action (a finished agent waiting for its
// world, a scripted agent, an absent slot) do not go through the network and are handed action 0 / value 0, what the step-by-step path's
// row-list pass leaves.  Every value is computed by the statements of the step-by-step path (cavoid_rollout_active_rows, policy_ws_forward_kernel /
// policy_wsring_forward_kernel on the row list, crowd_push_kernel) in the same order: trajectories, experience rings and episode logs are
// bit-identical to it (tests/test_gpu_crowd_ws_actor.py).  Nothing crosses workgroups; every loop is bounded by n_steps or M.
#pragma once
#include "cavoid_actor_ws.hpp"
#include "cavoid_crowd_actor.hpp"
#include "cavoid_policy_wsring.hpp"

namespace cavoid {

template <int NB, bool RVO>
__global__ void __launch_bounds__(256, 2) crowd_ws_rollout_kernel(const KCfg c, const KState s, const PoolRec *pool, const PolicyWsArgs wa_arg, const RolloutCfg rc,
                                                                  const RolloutState rs, const RolloutIO rio_arg, const ActorIO io, const int n) {
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
    const int64_t tile = blockIdx.x, w0 = tile * wpw, a0 = w0 * n;
    int64_t worlds_here = c.num_worlds - w0;
    worlds_here = worlds_here > wpw ? wpw : (worlds_here < 0 ? 0 : worlds_here);
    const int rows = (int)worlds_here * n;                   // policy rows = agent slots of this tile
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
            // actor_ws_kernel's predicate (cavoid_rollout_active_rows' on the step-by-step path): obs column 0 set, and the agent not done
            // in the step that produced this observation unless its world has just restarted; with the re-flush quirk every row counts
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
                // the live rows, in order, as the pass's row list (global rows: it gathers them from p.x and scatters the outputs; the ring's
                // refills go through the same list)
                if (wave_in_block == 0 && mine) tile_row[__popcll(live_mask & ((1ull << lane) - 1ull))] = (int)(a0 + lane);
                __syncthreads();
                PolicyWsArgs wa = wa_arg;
                wa.a.x = obs_t + 1;                          // column 0 (is_learning) is not a network input
                wa.a.v_out = io.values; wa.a.actions_out = io.actions; wa.a.greedy = io.greedy;
                policy_ws_forward_tile<false, kLossA3C, PolRing<kWsRing>, true>(wa, tid, n_live, pstep0 + t);
            }
        }
        __syncthreads();                                     // the tile's actions / values are in memory; the activation rows are idle

        // ---- env.step of the tile + the Experience bookkeeping of its slots on wavefront 0, the step's state rows -> the experience
        //      store on wavefronts 1..3; the mask of the rows that need an action at the next step -> live_next
        crowd_actor_env_phase<NB, RVO>(c, s, pool, rc, rs, rio_arg, io, obs_t, obs_n, lds_tab, wbase, live_next, n, wave_in_block, lane, tile, w0, a0,
                                       rows, step, blk);
        __syncthreads();                                     // obs(t+1), the world state, the slot state and live_next are in place
    }
}

}  // namespace cavoid
