// cavoid_eval.hpp -- eval_kernel<N, RVO, FROZEN>: the EVALUATION loop, K env steps in ONE launch, with a device-side outcome record.
//
// What ga3c/evaluate.py does per env step from the host (policy launch, cavoid_step, a copy of the world buffer, mask launches, a host
// synchronisation on `over.all()`), per tile of floor(64/N) worlds inside one workgroup of four wavefronts -- actor_kernel's launch
// shape (cavoid_actor.hpp) without the Experience bookkeeping:
//
//   all 4 wavefronts   NetworkVP_rnn forward of the tile's rows that still need an action (policy_split_tile) + argmax / Philox draw
//   wavefront 0        env.step of the tile WITHOUT auto-reset (env_tile<N, MODE_STEP>; or all four: quad_env_tile<N, false>), LDS lent by
//                      the idle activation planes; then the outcome recorder, one lane per agent slot
//
// Worlds never restart.  A tile whose worlds are all over leaves the step loop (evaluation episodes end between step 11 and step 295 of
// one round: most tile-steps of a fixed-length loop would be spent on worlds that ended long before), and on leaving reports how many
// of its worlds are still running, so that the host learns "everything is over" from one word per launch.  Nothing crosses
// workgroups, there is no polled wait, every loop is bounded by n_steps.  Every value is computed by the statements of the
// step-by-step entry points (cavoid_policy_forward, cavoid_step), so a round is bit-identical to one driven from the host
// (tests/test_gpu_eval_fused.py).
#pragma once
#include "cavoid_kernels.hpp"
#include "cavoid_quad.hpp"
#include "cavoid_policy_split.hpp"

namespace cavoid {

constexpr int kEvalQuadMaxAgents = 4;    // the cooperative env step inside the kernel: instantiated up to this many agents per world (as actor_kernel)

struct EvalIO {
    float *obs;               // [W,N,1+D]: the observation acted on AND, after the step, the next one (one buffer, see the kernel)
    float *rewards;           // [W,N]   the env's step outputs; they hold each tile's LAST step's afterwards
    uint8_t *done;            // [W,N]
    uint8_t *game_over;       // [W]
    int32_t *actions;         // [W,N]   select_action's choice (hand-over policy -> env inside a step)
    float *values;            // [W,N]
    double *ret;              // [W,N]   the records (cavoid_eval_buffers, include/cavoid.h)
    int32_t *goal_step;       // [W,N]
    int32_t *world_steps;     // [W]
    int32_t *worlds_running;  // [1]
    int32_t n_steps;
    int32_t greedy;
    int32_t quad;             // the tile's env step by all four wavefronts (the host sets it where actor_run would)
};

// the tile's records between the steps of a launch, behind the policy's LDS: registers live across the matrix phases would cost the
// policy pass its budget (and the kernel must take no scratch)
struct EvalShared {
    double ret[64];
    int32_t goal_step[64];
    int32_t world_steps[64];  // (per lane: its world's)
    int32_t running[2];       // ballot: the lane's world is NOT over
    int32_t live[2];          // ballot: the row needs an action at the next step
    int32_t over;             // no world of the tile is running: the workgroup leaves the step loop
    int32_t pad[3];
};
__host__ __device__ constexpr size_t eval_lds_bytes() { return ((policy_split_lds_bytes() + 15) & ~(size_t)15) + sizeof(EvalShared); }

// LDS the env step of a tile needs inside the (idle) activation planes (actor_env_lds_bytes' sum)
__host__ __device__ inline size_t eval_env_lds_bytes(int n_agents, int tile_floats, int rvo_floats = 0) {
    return (size_t)(lds_floats_block() + lds_floats_fixed(n_agents) + tile_floats + rvo_floats) * sizeof(float);
}

// The outcome recorder, on wavefront 0 behind the tile's env step (its lane mapping: one lane per agent slot): every agent of a world
// that was NOT over before this step adds the step's reward to its return (float64, in step order) and its world counts the step; an
// agent the step left at its goal for the first time notes the world's step count.  Then the masks the next step starts from.
__device__ __forceinline__ void eval_record(EvalShared &sh, const StepOut &so, bool in_range, int lane) {
    const unsigned long long was = (unsigned long long)(uint32_t)sh.running[0] | ((unsigned long long)(uint32_t)sh.running[1] << 32);
    if (in_range && ((was >> lane) & 1ull)) {
        sh.ret[lane] += (double)so.reward;
        const int32_t ws = sh.world_steps[lane] + 1;
        sh.world_steps[lane] = ws;
        if ((so.flags & CAVOID_F_AT_GOAL) && sh.goal_step[lane] == 0) sh.goal_step[lane] = ws;
    }
    const unsigned long long running = __ballot(in_range && !so.game_over);
    // (no restart here: a learning agent needs an action while it carries no terminal flag -- actor_kernel's predicate without its
    //  "or the world has just restarted")
    const unsigned long long live = __ballot(in_range && so.learning_next && !so.done);
    if (lane == 0) {
        sh.running[0] = (int)(uint32_t)running; sh.running[1] = (int)(uint32_t)(running >> 32);
        sh.live[0] = (int)(uint32_t)live; sh.live[1] = (int)(uint32_t)(live >> 32);
        sh.over = running == 0ull ? 1 : 0;
    }
}

template <int N, bool RVO, bool FROZEN = false>
__global__ void __launch_bounds__(256, 2) eval_kernel(const KCfg c, const KState s, const PoolRec *pool, const SplitArgs sa, const SplitArgs fz, const EvalIO io) {
    extern __shared__ __attribute__((aligned(16))) unsigned char planes[];      // the policy's activation planes ...
    float *len_f = reinterpret_cast<float *>(planes + 2 * kSpPlaneB);
    int *wave_max = reinterpret_cast<int *>(len_f + 64) + 64;
    int &ticket = wave_max[4];
    double *lds_tab = reinterpret_cast<double *>(planes);                        // ... lent to the env step while they are idle
    float *wbase = reinterpret_cast<float *>(planes) + lds_floats_block();
    EvalShared &sh = *reinterpret_cast<EvalShared *>(planes + ((policy_split_lds_bytes() + 15) & ~(size_t)15));

    const PolicyArgs &p = sa.p;
    const int tid0 = threadIdx.x;
    const int wpw = c.wpw, A = p.num_actions, ow = c.width;
    const int64_t tile = blockIdx.x, w0 = tile * wpw, a0 = w0 * N;
    int64_t worlds_here = c.num_worlds - w0;
    worlds_here = worlds_here > wpw ? wpw : (worlds_here < 0 ? 0 : worlds_here);
    const int rows = (int)worlds_here * N;                   // policy rows = agent slots of this tile
    const int32_t pstep0 = *p.step_counter;

    if (tid0 == 0) ticket = policy_cu_ticket(p.cu_tickets);   // arrival parity on the CU -> static priority (policy_cu_ticket, cavoid_policy.hpp)
    if (tid0 < 64) {
        // the tile's records, and which of its worlds are over -- env_tile's game_over predicate on the STATE's flags, so that a launch
        // on a finished tile does nothing (and a launch that begins on a part-finished tile goes on where the last one stopped)
        const int lw = tid0 / N;
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
        const int base = in_range ? lw * N : 0;
        const unsigned long long running = __ballot(in_range && (run_a & (((1ull << N) - 1ull) << base)) != 0ull);
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

        // ---- predict_p_and_v + select_action for the tile's rows, read in place from the observation the env wrote -----------
        {
            const float *src = obs + a0 * ow + 1;              // column 0 (is_learning) is not a network input
            auto load = [&](int r, int k) -> float { return src[(int64_t)r * ow + k]; };
            auto emit = [&](int trow, int g, const float (&pj)[4], const f32x4 &logit) {
                const int64_t row = a0 + trow;
                const int action = split_select_action(pj, g, lane, A, io.greedy != 0, row, pstep0 + t, p.seed_lo, p.seed_hi);
                if (trow < rows) {
                    if (g == 0) io.actions[row] = action;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (4 * g + r == A) io.values[row] = logit[r];
                }
            };
            if constexpr (!FROZEN) {
                // only the rows that still need an action go through the network (policy_split_tile, COMPACT): a learning agent whose
                // state carries no terminal flag; the env ignores what a finished or a scripted agent is given
                bool mine = lane < rows;
                if (t == 0) {                                // (uniform) the first step of a launch: from the WORLD STATE, as actor_kernel
                    if (mine) mine = obs[(a0 + lane) * ow] > 0.5f && (s.flags[a0 + lane] & CAVOID_F_DONE_MASK) == 0u;
                } else {                                     // the later ones: the mask the tile's own env step left in LDS
                    const unsigned long long m = (unsigned long long)(uint32_t)sh.live[0] | ((unsigned long long)(uint32_t)sh.live[1] << 32);
                    mine = (m >> lane) & 1ull;
                }
                // (a row that needs no action is handed action 0 / value 0)
                if (wave_in_block == 0 && lane < rows && !mine) { io.actions[a0 + lane] = 0; io.values[a0 + lane] = 0.0f; }
                const unsigned long long live_mask = __ballot(mine);
                const int n_rt = (__popcll(live_mask) + 15) >> 4;
                int *rmap = reinterpret_cast<int *>(len_f + 64);
                if (n_rt == 4) policy_split_tile<kSpDefaultProducts, 4>(sa, planes, len_f, wave_max, rows, tid, load, emit, live_mask, rmap);
                else if (n_rt == 3) policy_split_tile<kSpDefaultProducts, 3>(sa, planes, len_f, wave_max, rows, tid, load, emit, live_mask, rmap);
                else if (n_rt >= 1) policy_split_tile<kSpDefaultProducts, 2>(sa, planes, len_f, wave_max, rows, tid, load, emit, live_mask, rmap);
            } else {
                policy_split_tile<kSpDefaultProducts>(sa, planes, len_f, wave_max, rows, tid, load, emit);
                // the rows whose agent is a running frozen-network agent: the same pass on the frozen network's weights, its argmax (actor_kernel's)
                bool mine = false;
                if (tid < rows) {
                    const uint32_t f = s.flags[a0 + tid];
                    mine = (f & CAVOID_F_PRESENT) && ((f >> CAVOID_F_POLICY_SHIFT) & CAVOID_F_POLICY_MASK) == (uint32_t)CAVOID_POLICY_FROZEN_NET &&
                           (f & CAVOID_F_DONE_MASK) == 0u;
                }
                __syncthreads();                             // every wavefront is done with the learner's pass (planes, wave_max)
                if (tid < 64) { const unsigned long long m = __ballot(mine); if (lane == 0) { wave_max[12] = (int)(uint32_t)m; wave_max[13] = (int)(uint32_t)(m >> 32); } }
                __syncthreads();
                const unsigned long long frozen_rows = (unsigned long long)(uint32_t)wave_max[12] | ((unsigned long long)(uint32_t)wave_max[13] << 32);
                if (frozen_rows != 0ull) {                   // (uniform over the workgroup)
                    auto emit_fz = [&](int trow, int g, const float (&pj)[4], const f32x4 &) {
                        const int action = split_select_action(pj, g, lane, A, true, a0 + trow, 0, 0u, 0u);       // argmax: no random draw
                        if (trow < rows && g == 0 && ((frozen_rows >> trow) & 1ull)) io.actions[a0 + trow] = action;
                    };
                    policy_split_tile<kSpDefaultProducts>(fz, planes, len_f, wave_max, rows, tid, load, emit_fz);
                }
            }
        }
        // The tile's actions are in memory and the planes are idle -- and every wavefront is done READING the tile's observation rows:
        // there is no experience copy here, so the env step below writes the next observation into the very buffer the pass above
        // read (one buffer, no ping-pong).  This barrier is what makes that safe; the one at the end of the step orders the other way.
        __syncthreads();

        KIO k{};
        k.actions = io.actions; k.obs = obs; k.rew = io.rewards; k.done = io.done; k.game_over = io.game_over;
        k.obs_stride = ow; k.n_steps = 1;
        StepOut so{0.0f, true, true, false, 0u};
        if (!RVO && N <= kEvalQuadMaxAgents && io.quad) {    // (uniform) env.step of the tile by all four wavefronts (cavoid_quad.hpp), no restart
            quad_env_tile<(N <= kEvalQuadMaxAgents ? N : 1), false>(c, s, pool, k, planes, wave_in_block, lane, tile, &so);
            if (wave_in_block == 0) eval_record(sh, so, lane < rows, lane);
        } else if (wave_in_block == 0) {                     // ... or by wavefront 0: cavoid_step's statements
            env_tile<N, MODE_STEP, RVO>(c, s, pool, k, lds_tab, wbase, lane, tile, &so);
            eval_record(sh, so, lane < rows, lane);
        }
        __syncthreads();                                     // obs(t+1), the world state, the records and the masks are in place
    }

    // ---- on leaving: the records go back, and the tile says how many of its worlds are still running ----------------------------------
    if (tid0 < 64 && rows > 0) {
        const int lw = tid0 / N, i = tid0 - lw * N;
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

#ifdef CAVOID_EVAL_KERNELS       /* the non-template kernel is compiled by cavoid_eval.hip only */
// after the evaluation launch: the policy's step counter moves on by n_steps, so that sampled evaluation draws what the step-by-step path draws
__global__ void eval_finish_kernel(int32_t *policy_step, int32_t n_steps) { *policy_step += n_steps; }
#endif

}  // namespace cavoid
