// cavoid_crowd_push.hpp -- crowd_push_kernel<NB>: one auto-reset step of every crowd world (17..64 agents, cavoid_crowd.hpp) + that
// step's Experience bookkeeping and episode log in ONE launch -- step_push_kernel (cavoid_actor.hpp) for the crowd step form.  Three
// launches (crowd_kernel, rollout_push_kernel, rollout_episode_kernel) become one: the step's rewards, done flags and game_over go from
// the env step to the bookkeeping in registers, and the step's state rows -- the widest in the project, up to 64 x 452 floats per tile
// -- are copied into the experience store WHILE the env step runs, not by the bookkeeping wavefront in front of it.
//
// One workgroup of TWO wavefronts per tile (floor(64/n) worlds), sharing the one LDS allocation of crowd_kernel:
//   wavefront 0   env.step of the tile (crowd_tile<NB, MODE_STEP_AUTORESET_N>, one step: the instantiation cavoid_step_autoreset
//                 launches on a crowd env), then the bookkeeping of the tile's slots (rollout_push_slot) and the episode log
//                 (rollout_close_episode) -- the statements of actor_env_push_tile with the agent count taken at run time
//   wavefront 1   the tile's rows of the observation acted on -> x[blk] (rollout_copy_rows), then it returns.  It touches no LDS.
// crowd_tile synchronises at wavefront scope only (wave_lds_sync), so the two never meet at a barrier.  Why not step_push_kernel's
// second grid half for the copy: a launch's dynamic LDS is the same for every workgroup (19 KB at n = 17 .. 58 KB at n = 64), so
// copy-only workgroups would reserve it for nothing and take residency from the env workgroups (a CU holds two 58 KB workgroups).
// Every value is computed by the same statements in the same order as in the three launches: observations, world state, rings and
// episode records are bit-identical to them (tests/test_gpu_crowd_push.py; the episode totals are double atomics, order-free to 1e-6).
#pragma once
#include "cavoid_actor.hpp"
#include "cavoid_crowd.hpp"

namespace cavoid {

// The kernel's text, once for both env steps: crowd_tile<NB, MODE_STEP_AUTORESET_N, RVO> inside.  A macro and not a body function over RVO: the
// function, inlined, gives crowd_push_kernel another instruction stream (operand order, register numbers) than the kernel written out, and the
// kernels that exist keep theirs.
#define CAVOID_CROWD_PUSH_KERNEL(KERNEL, RVO)                                                                                                      \
    template <int NB>                                                                                                                              \
    __global__ void __launch_bounds__(128) KERNEL(const KCfg c, const KState s, const PoolRec *pool, const RolloutCfg rc, const RolloutState rs,   \
                                                  const RolloutIO rio_arg, const ActorIO io, const int n, const int32_t step_arg) {                \
        extern __shared__ __attribute__((aligned(16))) unsigned char smem[];                                                                       \
        const int wave_in_block = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;                             \
        const int64_t tile = blockIdx.x;                                                                                                           \
        const int32_t step = step_arg >= 0 ? step_arg : *io.rollout_step;                                                                          \
        const int blk = step % rc.ring_len;                                                                                                        \
        const int wpw = c.wpw, ow = c.width;                                                                                                       \
        const int64_t w0 = tile * wpw;                                                                                                             \
        const float *obs_t = io.obs[0];                                                                                                            \
        if (wave_in_block == 1) {                                                                                                                  \
            /* the step's state rows -> the time-major experience store (the rows are obs_cur, complete before the launch: nothing here depends */ \
            /* on the env step wavefront 0 runs).  rollout_copy_rows' multiply-shift index is exact: at most 64 x 452 values < 2^16. */            \
            int64_t worlds_here = c.num_worlds - w0;                                                                                               \
            worlds_here = worlds_here > wpw ? wpw : (worlds_here < 0 ? 0 : worlds_here);                                                           \
            rollout_copy_rows<CAVOID_COPY_U>(rc, obs_t, rio_arg.x, w0 * n, (int)worlds_here * n, blk, lane, 64);                                   \
            return;                                                                                                                                \
        }                                                                                                                                          \
        double *lds_tab = reinterpret_cast<double *>(smem);                                                                                        \
        float *wbase = reinterpret_cast<float *>(smem) + lds_floats_block();                                                                       \
        KIO k{};                                                                                                                                   \
        k.actions = io.actions; k.obs = io.obs[1]; k.rew = io.rewards; k.done = io.done; k.game_over = io.game_over;                               \
        k.obs_stride = ow; k.n_steps = 1;                        /* (out_step_stride = 0: the one step's outputs in slot 0) */                     \
        StepOut so{0.0f, true, false, false};                                                                                                      \
        const int lw = lane / n, i = lane - lw * n;                                                                                                \
        const int64_t w = w0 + lw, a = w * n + i;                                                                                                  \
        const bool in_range = lane < wpw * n && w < c.num_worlds;                                                                                  \
        /* the bookkeeping's first trip to memory, issued in front of the env step (see actor_env_push_tile) */                                    \
        const RolloutSlot slot_in = rollout_slot_load(rs, a, in_range);                                                                            \
        float learn_f = 0.0f, value = 0.0f;                      /* is_learning of the state acted on (ProcessAgent.py:130) */                     \
        int action = 0;                                                                                                                            \
        if (in_range) { learn_f = obs_t[a * ow]; value = io.values[a]; action = io.actions[a]; }                                                   \
        crowd_tile<NB, MODE_STEP_AUTORESET_N, RVO>(c, s, pool, k, n, lds_tab, wbase, lane, tile, &so);                                             \
        const bool learning = in_range && learn_f > 0.5f;                                                                                          \
        const int base = lane < wpw * n ? lw * n : 0;                                                                                              \
        const uint64_t wbits = n >= 64 ? ~0ull : ((1ull << n) - 1ull);       /* (crowd_tile's form: a shift by 64 is undefined) */                 \
        const int n_learning = __popcll(__ballot(learning) & (wbits << base));                                                                     \
        RolloutIO rio = rio_arg;                                                                                                                   \
        rollout_push_slot(rc, rs, rio, a, in_range ? w : 0, i, in_range, learning, n_learning, so.done, so.game_over, so.reward, value, action,    \
                          step, blk, slot_in);                                                                                                     \
        /* episode_log_q.put: the totals above were accumulated with atomics by this wavefront's own lanes -- drain them; */                       \
        /* rollout_close_episode reads the sums at the cache the atomics went to */                                                                \
        if (__ballot(in_range && so.game_over) != 0ull) {                                                                                          \
            __builtin_amdgcn_s_waitcnt(0);                       /* (vmcnt 0: the atomics have been performed at the L2) */                        \
            if (in_range && i == 0 && so.game_over) rollout_close_episode(rc, rs, rio, w);                                                         \
        }                                                                                                                                          \
    }

CAVOID_CROWD_PUSH_KERNEL(crowd_push_kernel, false)
// the same launch for an env whose worlds may hold ORCA agents (cfg.rvo_enabled = CAVOID_RVO_WAVE; instantiated in cavoid_crowd_rvo.hip)
CAVOID_CROWD_PUSH_KERNEL(crowd_rvo_push_kernel, true)
#undef CAVOID_CROWD_PUSH_KERNEL

}  // namespace cavoid
