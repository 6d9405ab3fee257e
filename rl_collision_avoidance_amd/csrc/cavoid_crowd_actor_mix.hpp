// cavoid_crowd_actor_mix.hpp -- crowd_mix_rollout_kernel<NB, RVO>: crowd_actor_kernel's step loop (cavoid_crowd_actor.hpp) for the reference's TRAINING
// MIX in crowd worlds (17..64 agents): the tile may hold frozen-network agents (scripted policy 4, CAVOID_POLICY_FROZEN_NET: NON-learning agents
// driven by a second, frozen NetworkVP_rnn -- the GA3C-CADRL agent of ga3c/GA3C/Server.py:36), and a second SplitArgs `fz` carries that network.
//
// Per step, after the learner's pass (the ring form on the whole tile whenever one row still needs an action, its result handed to those rows
// only) a tile with at least one RUNNING policy-4 agent runs the same ring pass once more on `fz` and takes its argmax for exactly those rows --
// actor_kernel<N, RVO, FROZEN = true>'s frozen pass (cavoid_actor.hpp) for the ring form, what BatchedRollout.act does with cavoid_policy_rows +
// cavoid_policy_forward_rows in the step-by-step path.  Which rows those are is read from the state's flags BEFORE this step; every wavefront
// reads the same 64 rows, so a ballot hands each of them the mask: no LDS word, wave_max[12..13] keeps the learner's live mask.  Tiles without such
// agents skip the second pass (one ballot per step).  The learner's pass stays skipped when no row is live; the frozen pass runs all the same.
//
// Everything else is crowd_actor_kernel's text: the env phase (crowd_actor_env_phase), the lane index made per step from nothing live
// (crowd_actor_lane_id), the prologue.  Trajectories, experience rings and episode logs are bit-identical to the step-by-step path
// (tests/test_gpu_crowd_actor_mix.py).
// (The kernel's name keeps clear of "actor_kernel", "crowd_kernel" and "crowd_ws_rollout_kernel": the host tests count instantiations by those.)
#pragma once
#include "cavoid_crowd_actor.hpp"

namespace cavoid {

// the tile's rows whose agent is a running frozen-network agent, from the env state's flags (this step has not run yet): the same mask on
// every wavefront
__device__ __forceinline__ unsigned long long crowd_mix_frozen_rows(const KState &s, const int64_t a0, const int rows, const int lane) {
    bool fzrow = false;
    if (lane < rows) {
        const uint32_t f = s.flags[a0 + lane];
        fzrow = (f & CAVOID_F_PRESENT) && ((f >> CAVOID_F_POLICY_SHIFT) & CAVOID_F_POLICY_MASK) == (uint32_t)CAVOID_POLICY_FROZEN_NET &&
                (f & CAVOID_F_DONE_MASK) == 0u;
    }
    return __ballot(fzrow);
}

template <int NB, bool RVO>
__global__ void __launch_bounds__(256, 2) crowd_mix_rollout_kernel(const KCfg c, const KState s, const PoolRec *pool, const SplitArgs sa, const SplitArgs fz,
                                                                   const RolloutCfg rc, const RolloutState rs, const RolloutIO rio_arg, const ActorIO io,
                                                                   const int n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char planes[];      // the policy's activation planes ...
    float *len_f = reinterpret_cast<float *>(planes + 2 * kSpPlaneB);
    int *wave_max = reinterpret_cast<int *>(len_f + 64) + 64;                    // ([12], [13]: the live mask -- behind the planes, the env step leaves it alone)
    int &ticket = wave_max[4];
    double *lds_tab = reinterpret_cast<double *>(planes);                        // ... lent to the env step while they are idle
    float *wbase = reinterpret_cast<float *>(planes) + lds_floats_block();

    const PolicyArgs &p = sa.p;
    const int tid0 = threadIdx.x;
    const int wave0 = __builtin_amdgcn_readfirstlane(tid0 >> 6);
    const int wpw = c.wpw, A = p.num_actions, ow = c.width;
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
        // the thread id re-materialised per step from nothing that lives in a vector register (crowd_actor_kernel's note)
        const int wave_in_block = wave0;
        int lane = crowd_actor_lane_id();
        const float *obs_t = io.obs[t & 1];
        float *obs_n = io.obs[(t + 1) & 1];
        const int32_t step = step0 + t;
        const int blk = step % rc.ring_len;

        // ---- predict_p_and_v + select_action for the tile's rows, read in place from the observation the env wrote -----------
        {
            // the rows that still need an action (crowd_actor_kernel's predicate); with the reference's re-flush quirk every row runs
            bool mine = lane < rows;
            if (rc.reflush_done == 0) {
                if (t == 0) {                                // (uniform) the first step of a launch: from the WORLD STATE (see actor_kernel)
                    if (mine) mine = obs_t[(a0 + lane) * ow] > 0.5f && (s.flags[a0 + lane] & CAVOID_F_DONE_MASK) == 0u;
                } else {                                     // the later ones the mask the tile's own env step left in LDS
                    const unsigned long long m = (unsigned long long)(uint32_t)wave_max[12] | ((unsigned long long)(uint32_t)wave_max[13] << 32);
                    mine = (m >> lane) & 1ull;
                }
            }
            // (a row that needs no action is handed action 0 / value 0, what the step-by-step path's row-list pass leaves there)
            if (wave_in_block == 0 && lane < rows && !mine) { io.actions[a0 + lane] = 0; io.values[a0 + lane] = 0.0f; }
            const unsigned long long live_mask = __ballot(mine);            // (every wavefront evaluates the same 64 rows: no trip through LDS)
            const unsigned long long frozen_rows = crowd_mix_frozen_rows(s, a0, rows, lane);     // (the same on every wavefront, too)
            const float *src = obs_t + a0 * ow + 1;                        // column 0 (is_learning) is not a network input
            auto load = [&](int r, int k) -> float { return src[(int64_t)r * ow + k]; };
            if (live_mask != 0ull) {                                       // (uniform over the workgroup; 0: nobody in the tile needs an action)
                const int tid = wave_in_block * 64 + lane;
                auto emit = [&](int trow, int g, const float (&pj)[4], const f32x4 &logit) {
                    const int64_t row = a0 + trow;
                    const int action = split_select_action(pj, g, lane, A, io.greedy != 0, row, pstep0 + t, p.seed_lo, p.seed_hi);
                    if (trow < rows && ((live_mask >> trow) & 1ull)) {      // (no compaction with the ring: the pass covers the tile, the live rows take its result)
                        if (g == 0) io.actions[row] = action;
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (4 * g + r == A) io.values[row] = logit[r];
                    }
                };
                // The softmax renormalises by 1 / (1 + min_policy * (float)A): uniform floats the compiler computes once, in front of the STEP loop,
                // and keeps in vector registers across both passes and the env phase -- for each network, and with two networks they went to
                // scratch (12 to 16 bytes per lane).  A copy of the arguments whose min_policy and num_actions the compiler cannot see through keeps
                // the conversion and the division inside the pass (crowd_actor_env_phase's measure for 1.0 / c.dt): the same operations on the same values.
                SplitArgs sa_t = sa;
                asm volatile("" : "+s"(sa_t.p.min_policy), "+s"(sa_t.p.num_actions));
                policy_split_tile<kSpDefaultProducts, 0, false, SpRing<kSpCrowdRing>>(sa_t, planes, len_f, wave_max, rows, tid, load, emit);
            }
            // ---- the frozen network's pass for the running policy-4 rows (actor_kernel<N, RVO, true>'s, ring form) ----------------
            if (frozen_rows != 0ull) {                                     // (uniform over the workgroup)
                __syncthreads();                                           // every wavefront is done with the learner's pass (planes, wave_max); its actions are in memory
                lane = crowd_actor_lane_id();                              // (made again: not carried across the pass)
                const int tid = wave_in_block * 64 + lane;
                auto emit_fz = [&](int trow, int g, const float (&pj)[4], const f32x4 &) {
                    const int action = split_select_action(pj, g, lane, A, true, a0 + trow, 0, 0u, 0u);       // argmax: no random draw
                    if (trow < rows && g == 0 && ((frozen_rows >> trow) & 1ull)) io.actions[a0 + trow] = action;
                };
                SplitArgs fz_t = fz;                                       // (as above: the frozen network's 1 / (1 + min_policy * A) stays inside its pass)
                asm volatile("" : "+s"(fz_t.p.min_policy), "+s"(fz_t.p.num_actions));
                policy_split_tile<kSpDefaultProducts, 0, false, SpRing<kSpCrowdRing>>(fz_t, planes, len_f, wave_max, rows, tid, load, emit_fz);
            }
        }
        __syncthreads();                                     // the tile's actions / values are in memory; the planes are idle
        lane = crowd_actor_lane_id();                        // (made again: not carried across the pass)

        // ---- env.step of the tile + the Experience bookkeeping of its slots on wavefront 0, the step's state rows -> the experience store
        //      on wavefronts 1..3; the next step's live mask at wave_max[12], [13]
        crowd_actor_env_phase<NB, RVO>(c, s, pool, rc, rs, rio_arg, io, obs_t, obs_n, lds_tab, wbase, wave_max + 12, n, wave_in_block, lane, tile, w0, a0,
                                       rows, step, blk);
        __syncthreads();                                     // obs(t+1), the world state and the slot state are in memory
    }
}

}  // namespace cavoid
