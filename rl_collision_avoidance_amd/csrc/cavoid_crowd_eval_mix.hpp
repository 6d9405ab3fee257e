// cavoid_crowd_eval_mix.hpp -- crowd_mix_evaluate_kernel<NB, RVO>: crowd_evaluate_kernel's step loop (cavoid_crowd_eval.hpp) for crowd worlds that hold
// frozen-network agents (scripted policy 4, CAVOID_POLICY_FROZEN_NET: NON-learning agents driven by a second, frozen NetworkVP_rnn), with a second
// SplitArgs `fz` for that network -- eval_kernel<N, RVO, FROZEN = true> (cavoid_eval.hpp) over the crowd launch shape.
//
// Per step, after the learner's pass a tile with at least one RUNNING policy-4 agent runs the ring pass once more on `fz` and takes its argmax
// for exactly those rows (crowd_mix_rollout_kernel's frozen pass, cavoid_crowd_actor_mix.hpp: the mask is a ballot over the state's flags before
// this step, the same on every wavefront; sh.live[] keeps the learner's live mask).  The learner's pass stays skipped when no row is live, and the
// frozen pass runs all the same: with evaluate_mode a frozen-network agent can outlive every learner of its tile.  Everything else is
// crowd_evaluate_kernel's text: the prologue, the early exit, the env step without auto-reset, the recorder (eval_record), the epilogue and the
// worlds_running protocol.  A round is bit-identical to one driven from the host with cavoid_policy_forward, cavoid_policy_forward_rows on the
// frozen handle and cavoid_step (tests/test_gpu_crowd_eval_mix.py).
// (The kernel's name keeps clear of "eval_kernel", "crowd_kernel", "crowd_evaluate_kernel" and "crowd_ws_evaluate_kernel": the host tests count
// instantiations by those.)
#pragma once
#include "cavoid_crowd_actor_mix.hpp"
#include "cavoid_crowd_eval.hpp"

namespace cavoid {

template <int NB, bool RVO>
__global__ void __launch_bounds__(256, 2) crowd_mix_evaluate_kernel(const KCfg c, const KState s, const PoolRec *pool, const SplitArgs sa, const SplitArgs fz,
                                                                    const EvalIO io, const int n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char planes[];      // the policy's activation planes ...
    float *len_f = reinterpret_cast<float *>(planes + 2 * kSpPlaneB);
    int *wave_max = reinterpret_cast<int *>(len_f + 64) + 64;
    int &ticket = wave_max[4];
    double *lds_tab = reinterpret_cast<double *>(planes);                        // ... lent to the env step while they are idle
    float *wbase = reinterpret_cast<float *>(planes) + lds_floats_block();
    EvalShared &sh = *reinterpret_cast<EvalShared *>(planes + ((policy_split_lds_bytes() + 15) & ~(size_t)15));

    const PolicyArgs &p = sa.p;
    const int tid0 = threadIdx.x;
    const int wave0 = __builtin_amdgcn_readfirstlane(tid0 >> 6);
    const int wpw = c.wpw, A = p.num_actions, ow = c.width;
    const int64_t tile = blockIdx.x, w0 = tile * wpw, a0 = w0 * n;
    int64_t worlds_here = c.num_worlds - w0;
    worlds_here = worlds_here > wpw ? wpw : (worlds_here < 0 ? 0 : worlds_here);
    const int rows = (int)worlds_here * n;                   // policy rows = agent slots of this tile
    const int32_t pstep0 = *p.step_counter;

    if (tid0 == 0) ticket = policy_cu_ticket(p.cu_tickets);   // arrival parity on the CU -> static priority (policy_cu_ticket, cavoid_policy.hpp)
    if (tid0 < 64) {
        // the tile's records, and which of its worlds are over (crowd_evaluate_kernel's prologue)
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
        // EARLY EXIT (crowd_evaluate_kernel's): one LDS word, uniform over the workgroup
        if (__builtin_amdgcn_readfirstlane(sh.over) != 0) break;
        // the thread id re-materialised per step from nothing that lives in a vector register (crowd_actor_kernel's note)
        const int wave_in_block = wave0;
        int lane = crowd_actor_lane_id();
        float *obs = io.obs;

        // ---- predict_p_and_v + select_action for the tile's rows, read in place from the observation the env wrote -----------
        {
            // the rows that still need an action (eval_kernel's predicate: a learning agent whose state carries no terminal flag; no restart here)
            bool mine = lane < rows;
            if (t == 0) {                                    // (uniform) the first step of a launch: from the WORLD STATE
                if (mine) mine = obs[(a0 + lane) * ow] > 0.5f && (s.flags[a0 + lane] & CAVOID_F_DONE_MASK) == 0u;
            } else {                                         // the later ones: the mask the tile's own env step left in LDS
                const unsigned long long m = (unsigned long long)(uint32_t)sh.live[0] | ((unsigned long long)(uint32_t)sh.live[1] << 32);
                mine = (m >> lane) & 1ull;
            }
            // (a row that needs no action is handed action 0 / value 0)
            if (wave_in_block == 0 && lane < rows && !mine) { io.actions[a0 + lane] = 0; io.values[a0 + lane] = 0.0f; }
            const unsigned long long live_mask = __ballot(mine);            // (every wavefront evaluates the same 64 rows: no trip through LDS)
            const unsigned long long frozen_rows = crowd_mix_frozen_rows(s, a0, rows, lane);     // (the same on every wavefront, too)
            const float *src = obs + a0 * ow + 1;                          // column 0 (is_learning) is not a network input
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
            // ---- the frozen network's pass for the running policy-4 rows (crowd_mix_rollout_kernel's) -------------------------------
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
        // The tile's actions are in memory and the planes are idle -- and every wavefront is done READING the tile's observation rows: the
        // env step below writes the next observation into the very buffer the passes above read (one buffer, no ping-pong, as eval_kernel).
        __syncthreads();
        lane = crowd_actor_lane_id();                        // (made again: not carried across the pass)

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

    // ---- on leaving: the records go back, and the tile says how many of its worlds are still running ----------------------------------
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
