// cavoid_crowd_actor.hpp -- crowd_actor_kernel<NB, RVO>: the GA3C actor's CLOSED loop for crowd worlds (17..64 agents, cavoid_crowd.hpp), K env
// steps in ONE launch -- actor_kernel (cavoid_actor.hpp) for the crowd step form.
//
// A crowd tile is floor(64/n) worlds x n agents <= 64 rows: exactly one 64-row policy tile.  One workgroup of four wavefronts per tile runs,
// per step and without leaving the launch:
//
//   all 4 wavefronts   NetworkVP_rnn forward of the tile's rows with the input slots as a ring (policy_split_tile<.., SpRing<kSpCrowdRing>>: the
//                      statements of policy_crowd_forward_kernel; rows of up to 63 observed neighbours) + the Philox action draw
//   wavefront 0        env.step of the tile (crowd_tile<NB, MODE_STEP_AUTORESET_N, RVO>, one step, its LDS carved out of the idle activation
//                      planes: at most 64 KB of their 66 KB), then the Experience bookkeeping of the tile's slots and the episode log -- the
//                      statements of crowd_push_kernel's wavefront 0
//   wavefronts 1..3    meanwhile: the step's state rows -> the time-major experience ring (rollout_copy_rows); they touch no LDS
//
// crowd_tile synchronises at wavefront scope only, so the env wavefront and the copying ones never meet inside the phase.  The ring pass has no
// row compaction (policy_split_tile: the ring is carried by the plain four-wavefront pass): the pass runs on the whole tile whenever one row
// still needs an action, and emit() hands the result to those rows only; a tile without such a row skips the pass.  State between the phases
// travels through global memory (same CU, workgroup barrier), exactly as in actor_kernel.  Every value is computed by the same statements in
// the same order as in the step-by-step path (row list, policy_crowd_forward_kernel / policy_forward_split_kernel, crowd_push_kernel):
// trajectories, experience rings and episode logs are bit-identical to it (tests/test_gpu_crowd_actor.py).
// Its own copy of the text it shares with actor_kernel and crowd_push_kernel: those kernels keep their instruction streams.
#pragma once
#include "cavoid_actor.hpp"
#include "cavoid_crowd.hpp"
#include "cavoid_policy_crowd.hpp"

namespace cavoid {

// LDS the crowd env step of a tile needs inside the (idle) activation planes: the action table + the wavefront's arrays (crowd_kernel's allocation)
__host__ __device__ inline size_t crowd_actor_env_lds_bytes(int n, int tile_rows, int ostride) {
    return (size_t)(lds_floats_block() + crowd_wave_floats(n, tile_rows, ostride)) * sizeof(float);
}

// this lane's index in its wavefront, from no live register: v_mbcnt over an all-ones mask, seeded with a zero the compiler cannot see through
// (two calls are two computations: nothing is kept between them)
__device__ __forceinline__ int crowd_actor_lane_id() {
    int z = 0;
    asm volatile("" : "+v"(z));
    return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)z));
}

// The env half of a crowd actor step, shared by crowd_actor_kernel and crowd_ws_rollout_kernel (cavoid_crowd_actor_ws.hpp): wavefront 0 runs env.step
// of the tile (its LDS at lds_tab / wbase, inside the policy's idle activation memory), then the Experience bookkeeping of the tile's slots
// and the episode log -- the statements of crowd_push_kernel's wavefront 0 -- and leaves the mask of the rows that need an action at the
// NEXT step in live_next[0..1] (LDS the env step does not reach); wavefronts 1..3 meanwhile copy the step's state rows into the time-major
// experience ring (they touch no LDS).  Between the caller's two workgroup barriers.
template <int NB, bool RVO>
__device__ __forceinline__ void crowd_actor_env_phase(const KCfg &c, const KState &s, const PoolRec *pool, const RolloutCfg &rc, const RolloutState &rs,
                                                      const RolloutIO &rio_arg, const ActorIO &io, const float *obs_t, float *obs_n, double *lds_tab,
                                                      float *wbase, int *live_next, const int n, const int wave_in_block, const int lane,
                                                      const int64_t tile, const int64_t w0, const int64_t a0, const int rows, const int32_t step,
                                                      const int blk) {
    const int wpw = c.wpw, ow = c.width;
    if (wave_in_block == 0) {
        // ---- env.step of the tile, then the Experience bookkeeping of its slots: crowd_push_kernel's wavefront 0 ----------------
        KIO k{};
        k.actions = io.actions; k.obs = obs_n; k.rew = io.rewards; k.done = io.done; k.game_over = io.game_over;
        k.obs_stride = ow; k.n_steps = 1;                    /* (out_step_stride = 0: the one step's outputs in slot 0) */
        StepOut so{0.0f, true, false, false};
        const int lw = lane / n, i = lane - lw * n;
        const int64_t w = w0 + lw, a = w * n + i;
        const bool in_range = lane < wpw * n && w < c.num_worlds;
        // the bookkeeping's first trip to memory, issued in front of the env step (see actor_env_push_tile)
        const RolloutSlot slot_in = rollout_slot_load(rs, a, in_range);
        float learn_f = 0.0f, value = 0.0f;                  // is_learning of the state acted on (ProcessAgent.py:130)
        int action = 0;
        if (in_range) { learn_f = obs_t[a * ow]; value = io.values[a]; action = io.actions[a]; }
        if constexpr (RVO) {
            // The ORCA solve divides by c.dt (1.0 / c.dt, cavoid_crowd_rvo.hpp).  c is a kernel argument, so the quotient is invariant
            // and was hoisted out of the STEP loop into a vector register pair live across the policy pass: 8 bytes of scratch per lane.
            // A copy of the configuration whose dt the compiler cannot see through keeps the division inside the env phase -- the
            // same operation on the same value; every other field is still read from the kernel arguments where it is used.
            KCfg cc = c;
            asm volatile("" : "+s"(cc.dt));
            crowd_tile<NB, MODE_STEP_AUTORESET_N, RVO>(cc, s, pool, k, n, lds_tab, wbase, lane, tile, &so);
        } else {
            crowd_tile<NB, MODE_STEP_AUTORESET_N, RVO>(c, s, pool, k, n, lds_tab, wbase, lane, tile, &so);
        }
        {   // the rows that need an action at the NEXT step, for the next policy pass: in LDS (behind the lent memory)
            const unsigned long long m = __ballot(in_range && so.learning_next && (so.game_over || !so.done));
            if (lane == 0) { live_next[0] = (int)(uint32_t)m; live_next[1] = (int)(uint32_t)(m >> 32); }
        }
        const bool learning = in_range && learn_f > 0.5f;
        const int base = lane < wpw * n ? lw * n : 0;
        const uint64_t wbits = n >= 64 ? ~0ull : ((1ull << n) - 1ull);       // (crowd_tile's form: a shift by 64 is undefined)
        const int n_learning = __popcll(__ballot(learning) & (wbits << base));
        RolloutIO rio = rio_arg;
        rollout_push_slot(rc, rs, rio, a, in_range ? w : 0, i, in_range, learning, n_learning, so.done, so.game_over, so.reward, value, action,
                          step, blk, slot_in);
        // episode_log_q.put: the totals above were accumulated with atomics by this wavefront's own lanes -- drain them;
        // rollout_close_episode reads the sums at the cache the atomics went to
        if (__ballot(in_range && so.game_over) != 0ull) {
            __builtin_amdgcn_s_waitcnt(0);                   // (vmcnt 0: the atomics have been performed at the L2)
            if (in_range && i == 0 && so.game_over) rollout_close_episode(rc, rs, rio, w);
        }
    } else {
        // ---- meanwhile: the step's state rows -> the time-major experience store -----------------------------------------
        rollout_copy_rows(rc, obs_t, rio_arg.x, a0, rows, blk, (wave_in_block - 1) * 64 + lane, 192);
    }
}

template <int NB, bool RVO>
__global__ void __launch_bounds__(256, 2) crowd_actor_kernel(const KCfg c, const KState s, const PoolRec *pool, const SplitArgs sa, const RolloutCfg rc,
                                                             const RolloutState rs, const RolloutIO rio_arg, const ActorIO io, const int n) {
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
        // The thread id re-materialised per step (see actor_kernel: each phase keeps the register footprint of its stand-alone kernel) -- and
        // here from NOTHING that lives in a vector register: the wavefront's index is uniform (a scalar register) and the lane index is
        // v_mbcnt of an opaque zero.  The ring pass leaves no vector register over at two workgroups per CU: with the id carried across
        // the loop and across the pass as in actor_kernel, both copies went to scratch (8 to 20 bytes per lane).
        const int wave_in_block = wave0;
        int lane = crowd_actor_lane_id();
        const int tid = wave_in_block * 64 + lane;
        const float *obs_t = io.obs[t & 1];
        float *obs_n = io.obs[(t + 1) & 1];
        const int32_t step = step0 + t;
        const int blk = step % rc.ring_len;

        // ---- predict_p_and_v + select_action for the tile's rows, read in place from the observation the env wrote -----------
        {
            // the rows that still need an action (actor_kernel's predicate: what cavoid_rollout_active_rows lists for the step-by-step path);
            // with the reference's re-flush quirk a done agent's value IS read: every row runs
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
            if (live_mask != 0ull) {                                       // (uniform over the workgroup; 0: nobody in the tile needs an action)
                const float *src = obs_t + a0 * ow + 1;                    // column 0 (is_learning) is not a network input
                auto load = [&](int r, int k) -> float { return src[(int64_t)r * ow + k]; };
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
                policy_split_tile<kSpDefaultProducts, 0, false, SpRing<kSpCrowdRing>>(sa, planes, len_f, wave_max, rows, tid, load, emit);
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
