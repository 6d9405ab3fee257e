// cavoid_crowd_eval_ws.hpp -- crowd_ws_evaluate_kernel<NB, RVO, FROZEN>: the EVALUATION loop for crowd worlds (17..64 agents, cavoid_crowd.hpp)
// and the weight-sharing network (MULTI_AGENT_ARCH 'weight_sharing'), K env steps in ONE launch with a device-side outcome record --
// cavoid_crowd_eval_run_ws.
//
// eval_ws_kernel's step loop (cavoid_eval_ws.hpp) over crowd_ws_rollout_kernel's launch shape and policy phase (cavoid_crowd_actor_ws.hpp),
// with crowd_evaluate_kernel's env phase (cavoid_crowd_eval.hpp) -- a new composition of their statements.  A crowd tile is floor(64/n)
// worlds x n agents <= 64 rows: one 64-row policy tile.  One workgroup of four wavefronts per tile runs, up to K times:
//
//   all 4 wavefronts   policy_ws_forward_tile<false, kLossA3C, PolRing<kWsRing>, true>: the float32-MFMA weight-sharing pass of the tile's rows
//                      that still need an action -- compacted into the pass's row list -- with the R = 19 input slots as a ring (rows of up
//                      to 63 observed neighbours), + argmax / the Philox draw -> actions / values of the tile
//   wavefront 0        env.step of the tile WITHOUT auto-reset (crowd_tile<NB, MODE_STEP, RVO>, its LDS carved out of the pass's activation
//                      rows, which are idle now), then the outcome recorder (eval_record, cavoid_eval.hpp), one lane per agent slot
//   wavefronts 1..3    wait at the closing barrier: there is no experience copy here
//
// LDS is eval_ws_kernel's map (eval_ws_lds_bytes() = 72 064 B, two workgroups per CU):
//   [0, 66 560)        the activation rows [64][kPolStride] -- LENT to the env step between two passes: the action table at 0, the wavefront's
//                      arrays behind it (crowd_kernel's allocation, at most 64 KB; the host checks crowd_actor_env_lds_bytes against both)
//   [66 560, 70 720)   the packed biases (rewritten by every pass)
//   [70 720, 70 752)   8 ints: [4] the CU ticket
//   [70 752, 71 008)   the pass's row list
//   [71 008, 72 064)   EvalShared: the tile's records and masks between the steps of a launch -- behind the row list, so that neither the
//                      pass nor the env step's scratch can reach it (the static_asserts of cavoid_eval_ws.hpp and the one below)
//
// ONE ring instantiation serves every neighbour count (crowd_ws_rollout_kernel's note): a cavoid_policy_create_ws handle (M <= 19) and a
// _create_ws_crowd handle (20..64) share ws_layout(M).  Unlike crowd_evaluate_kernel's ring pass this one IS compacted: a finished agent, a
// scripted agent and an absent slot do not go through the network and are handed action 0 / value 0.  FROZEN: the frozen-network agents
// (scripted policy 4) that are still running get a second row-list pass on the frozen handle's weights, argmax (eval_ws_kernel's second
// pass, through the same ring instantiation); values[] of those rows then holds the FROZEN network's value -- nothing reads it.  Worlds
// never restart.  A tile whose worlds are all over leaves the step loop and reports on leaving how many of its worlds are still running
// (eval_kernel's protocol).  Nothing crosses workgroups, there is no polled wait, every loop is bounded by n_steps or M.  Every value is
// computed by the statements of the step-by-step entry points (cavoid_policy_forward / _forward_rows on the weight-sharing handle,
// cavoid_step), so a round is bit-identical to one driven from the host (tests/test_gpu_crowd_ws_eval.py).
// (The kernel's name keeps clear of "eval_kernel", "eval_ws_kernel", "actor_kernel", "actor_ws_kernel", "crowd_kernel",
// "crowd_evaluate_kernel" and "crowd_ws_rollout_kernel": the host tests count instantiations by those.)
#pragma once
#include "cavoid_crowd_actor_ws.hpp"
#include "cavoid_eval_ws.hpp"

namespace cavoid {

// the env step's scratch ends inside the lent rows (the host refuses an env whose crowd step takes more than min(64 KB, the lent rows)),
// and EvalShared begins behind the biases, the ticket ints and the row list
static_assert(eval_ws_shared_offset() >= actor_ws_lent_bytes() + (kBiasFloats + 8 + 64) * sizeof(float) && actor_ws_lent_bytes() >= 65536,
              "EvalShared lies behind everything the crowd env step may write");

template <int NB, bool RVO, bool FROZEN>
__global__ void __launch_bounds__(256, 2) crowd_ws_evaluate_kernel(const KCfg c, const KState s, const PoolRec *pool, const PolicyWsArgs wa_arg,
                                                                   const PolicyWsArgs fz_arg, const EvalIO io, const int n) {
    extern __shared__ __attribute__((aligned(16))) float act[];                  // the pass's activation rows ...
    int *ticket_slot = ws_ticket_slot(act);
    int &ticket = ticket_slot[4];
    int *tile_row = ws_tile_row(act);
    double *lds_tab = reinterpret_cast<double *>(act);                           // ... lent to the env step while they are idle
    float *wbase = act + lds_floats_block();
    EvalShared &sh = *reinterpret_cast<EvalShared *>(reinterpret_cast<unsigned char *>(act) + eval_ws_shared_offset());

    const PolicyArgs &p = wa_arg.a;
    const int tid0 = threadIdx.x;
    const int wpw = c.wpw, ow = c.width;
    const int64_t tile = blockIdx.x, w0 = tile * wpw, a0 = w0 * n;
    int64_t worlds_here = c.num_worlds - w0;
    worlds_here = worlds_here > wpw ? wpw : (worlds_here < 0 ? 0 : worlds_here);
    const int rows = (int)worlds_here * n;                   // policy rows = agent slots of this tile
    const int32_t pstep0 = *p.step_counter;

    if (tid0 == 0) ticket = policy_cu_ticket(p.cu_tickets);   // arrival parity on the CU -> static priority (policy_cu_ticket, cavoid_policy.hpp)
    if (tid0 < 64) {
        // the tile's records, and which of its worlds are over -- crowd_tile's game_over predicate on the STATE's flags, so that a launch
        // on a finished tile does nothing (and a launch that begins on a part-finished tile goes on where the last one stopped):
        // crowd_evaluate_kernel's
        const int lw = tid0 / n;
        const bool in_range = tid0 < rows;
        uint32_t f = 0u;
        if (in_range) {
            f = s.flags[a0 + tid0];
            sh.ret[tid0] = io.ret[a0 + tid0];
            sh.goal_step[tid0] = io.goal_step[a0 + tid0];
            sh.world_steps[tid0] = io.world_steps[w0 + lw];
        }
        const unsigned long long run_a = __ballot(in_range && (f & CAVOID_F_PRESENT) && ((f & CAVOID_F_LEARNING) || c.evaluate_mode) &&
                                                  (f & CAVOID_F_DONE_MASK) == 0u);
        const int base = in_range ? lw * n : 0;
        const unsigned long long wbits = n >= 64 ? ~0ull : ((1ull << n) - 1ull);      // (crowd_tile's form: a shift by 64 is undefined)
        const unsigned long long running = __ballot(in_range && (run_a & (wbits << base)) != 0ull);
        if (tid0 == 0) {
            sh.running[0] = (int)(uint32_t)running; sh.running[1] = (int)(uint32_t)(running >> 32);
            sh.live[0] = sh.live[1] = 0;
            sh.over = running == 0ull ? 1 : 0;
        }
    }
    __syncthreads();
    if (ticket & 1) __builtin_amdgcn_s_setprio(1);

#pragma unroll 1
    for (int t = 0; t < io.n_steps; ++t) {
        // EARLY EXIT: one LDS word, written by wavefront 0 in front of the barrier that ended the last step (or the one above), read by
        // every thread behind it: the decision is uniform over the workgroup, so no barrier below is reached by part of it
        if (__builtin_amdgcn_readfirstlane(sh.over) != 0) break;
        // (the thread id re-materialised per step: actor_kernel's note on hoisting)
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const int wave_in_block = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        float *obs = io.obs;

        // ---- predict_p_and_v + select_action for the tile's rows that still need an action, read in place from the observation the env wrote
        {
            // eval_kernel's predicate: a learning agent whose state carries no terminal flag
            bool mine = lane < rows;
            if (t == 0) {                                    // (uniform) the first step of a launch: from the WORLD STATE
                if (mine) mine = obs[(a0 + lane) * ow] > 0.5f && (s.flags[a0 + lane] & CAVOID_F_DONE_MASK) == 0u;
            } else {                                         // the later ones: the mask the tile's own env step left in LDS
                const unsigned long long m = (unsigned long long)(uint32_t)sh.live[0] | ((unsigned long long)(uint32_t)sh.live[1] << 32);
                mine = (m >> lane) & 1ull;
            }
            // FROZEN: the rows whose agent is a running frozen-network agent (eval_kernel's predicate, on the state the last env step
            // left -- behind the barrier that ended it)
            bool theirs = false;
            if constexpr (FROZEN) {
                if (lane < rows) {
                    const uint32_t f = s.flags[a0 + lane];
                    theirs = (f & CAVOID_F_PRESENT) && ((f >> CAVOID_F_POLICY_SHIFT) & CAVOID_F_POLICY_MASK) == (uint32_t)CAVOID_POLICY_FROZEN_NET &&
                             (f & CAVOID_F_DONE_MASK) == 0u;
                }
            }
            // (a row that needs no action is handed action 0 / value 0, what the step-by-step path's row-list pass leaves there)
            if (wave_in_block == 0 && lane < rows && !mine && !theirs) { io.actions[a0 + lane] = 0; io.values[a0 + lane] = 0.0f; }
            const unsigned long long live_mask = __ballot(mine);            // (every wavefront evaluates the same 64 rows: no trip through LDS)
            const int n_live = __popcll(live_mask);
            if (n_live > 0) {                                // (uniform over the workgroup; 0: nobody in the tile needs the learner's action)
                // the live rows, in order, as the pass's row list (global rows: it gathers them from p.x and scatters the outputs; the
                // ring's refills go through the same list).  The list's last readers were the heads of the last step's pass: two barriers ago
                if (wave_in_block == 0 && mine) tile_row[__popcll(live_mask & ((1ull << lane) - 1ull))] = (int)(a0 + lane);
                __syncthreads();
                PolicyWsArgs wa = wa_arg;
                wa.a.x = obs + 1;                            // column 0 (is_learning) is not a network input
                wa.a.v_out = io.values; wa.a.actions_out = io.actions; wa.a.greedy = io.greedy;
                policy_ws_forward_tile<false, kLossA3C, PolRing<kWsRing>, true>(wa, tid, n_live, pstep0 + t);
            }
            if constexpr (FROZEN) {
                const unsigned long long frozen_mask = __ballot(theirs);
                const int n_frozen = __popcll(frozen_mask);
                if (n_frozen > 0) {                          // (uniform over the workgroup)
                    // the same pass on the frozen network's weights, its argmax.  It reuses the row list, the activation rows and the
                    // packed biases, which the heads of the learner's pass may still be reading: every wavefront is done with that pass
                    // behind this barrier (where there was no learner's pass it orders nothing and costs one barrier)
                    __syncthreads();
                    if (wave_in_block == 0 && theirs) tile_row[__popcll(frozen_mask & ((1ull << lane) - 1ull))] = (int)(a0 + lane);
                    __syncthreads();                         // the frozen rows' list is in place
                    PolicyWsArgs fa = fz_arg;
                    fa.a.x = obs + 1;
                    fa.a.v_out = io.values; fa.a.actions_out = io.actions; fa.a.greedy = 1;      // argmax: no random draw, the step keys nothing
                    policy_ws_forward_tile<false, kLossA3C, PolRing<kWsRing>, true>(fa, tid, n_frozen, 0);
                }
            }
        }
        // The tile's actions are in memory and the activation rows are idle -- and every wavefront is done READING the tile's observation
        // rows: the env step below writes the next observation into the very buffer the pass above read (one buffer, no ping-pong, as
        // eval_ws_kernel).  This barrier is what makes that safe; the one at the end of the step orders the other way.
        __syncthreads();

        if (wave_in_block == 0) {
            // ---- env.step of the tile without auto-reset (cavoid_step's statements), then the outcome recorder ----------------------
            KIO k{};
            k.actions = io.actions; k.obs = obs; k.rew = io.rewards; k.done = io.done; k.game_over = io.game_over;
            k.obs_stride = ow; k.n_steps = 1;
            StepOut so{0.0f, true, true, false, 0u};
            if constexpr (RVO) {
                // (crowd_actor_kernel's note: a copy of the configuration whose dt the compiler cannot see through keeps the ORCA solve's
                //  1.0 / c.dt inside the env phase -- the same operation on the same value)
                KCfg cc = c;
                asm volatile("" : "+s"(cc.dt));
                crowd_tile<NB, MODE_STEP, RVO>(cc, s, pool, k, n, lds_tab, wbase, lane, tile, &so);
            } else {
                crowd_tile<NB, MODE_STEP, RVO>(c, s, pool, k, n, lds_tab, wbase, lane, tile, &so);
            }
            eval_record(sh, so, lane < rows, lane);
        }
        __syncthreads();                                     // obs(t+1), the world state, the records and the masks are in place
    }

    // ---- on leaving: the records go back, and the tile says how many of its worlds are still running (crowd_evaluate_kernel's) --------
    if (tid0 < 64 && rows > 0) {
        const int lw = tid0 / n, i = tid0 - lw * n;
        if (tid0 < rows) {
            io.ret[a0 + tid0] = sh.ret[tid0];
            io.goal_step[a0 + tid0] = sh.goal_step[tid0];
            if (i == 0) io.world_steps[w0 + lw] = sh.world_steps[tid0];
        }
        const unsigned long long running = (unsigned long long)(uint32_t)sh.running[0] | ((unsigned long long)(uint32_t)sh.running[1] << 32);
        const int n_running = __popcll(__ballot(tid0 < rows && i == 0 && ((running >> tid0) & 1ull)));
        if (tid0 == 0 && n_running > 0) atomicAdd(io.worlds_running, n_running);     // (device scope; the host zeroed the word on the stream)
    }
}

}  // namespace cavoid
