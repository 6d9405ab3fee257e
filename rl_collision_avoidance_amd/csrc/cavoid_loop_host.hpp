// cavoid_loop_host.hpp -- the host path of a step-loop launch, once: what the eleven closed-loop entry points (cavoid_actor_run*,
// cavoid_crowd_actor_run*, cavoid_eval_run*, cavoid_crowd_eval_run*) and cavoid_step_push have in common around their kernels -- the
// argument checks, the kernel-argument fills, the launch of a kernel whose dynamic LDS is above 64 KiB, and the crowd launches' prologue
// and bucket.  An entry point keeps its own ordered list of refusals (each form's contract: the tests and the Python reason functions
// mirror it one for one) and then reads: shared fills, one launch call, the finish kernel.  What distinguishes the forms is an argument
// at the call site: the LDS the policy pass lends the env step (`lent`), whether a look-ahead env is refused (`refuse_ahead`), whether
// the env step streams its observation rows (`stream_obs`), the frozen network's rule (frozen_split_args / frozen_ws_args), and whether
// the look-ahead rings are prepared (loop_ahead_prepare: the actor forms and cavoid_step_push; an evaluation restarts nothing).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "cavoid.h"
#include "cavoid_crowd_actor.hpp"
#include "cavoid_eval.hpp"
#include "cavoid_host.hpp"
#include "cavoid_launch.hpp"
#include "cavoid_policy_host.hpp"
#include "cavoid_rollout_host.hpp"

namespace cavoid {

// ---- argument checks (every failure is CAVOID_EINVAL) -----------------------------------------------------------------------------------
inline bool rollout_buffers_ok(const cavoid_rollout_buffers *b) {
    return b && b->struct_size == (int32_t)sizeof(cavoid_rollout_buffers) && b->x && b->val && b->ret && b->act && b->emit_t && b->dup_x && b->dup_r &&
           b->dup_a && b->dup_src && b->dup_count && b->ep_out && b->ep_count && b->dup_capacity >= 1 && b->ep_capacity >= 1;
}

inline bool eval_buffers_ok(const cavoid_eval_buffers *b) {
    return b && b->struct_size == (int32_t)sizeof(cavoid_eval_buffers) && b->ret && b->goal_step && b->world_steps && b->worlds_running;
}

// the pointers and the step count of the actor signature (a form with a required `frozen` checks that one itself)
inline bool actor_args_ok(const cavoid_env *e, const cavoid_policy *h, const cavoid_rollout *r, const cavoid_rollout_buffers *b, const float *obs_cur,
                          const float *obs_next, const float *rewards, const uint8_t *done, const uint8_t *game_over, const int32_t *actions,
                          const float *values, int32_t n_steps) {
    return e && h && r && obs_cur && obs_next && obs_cur != obs_next && rewards && done && game_over && actions && values && n_steps >= 0 &&
           rollout_buffers_ok(b);
}

// ... and of the evaluation signature
inline bool eval_args_ok(const cavoid_env *e, const cavoid_policy *h, const cavoid_eval_buffers *b, const float *obs, const float *rewards,
                         const uint8_t *done, const uint8_t *game_over, const int32_t *actions, const float *values, int32_t n_steps) {
    return e && h && obs && rewards && done && game_over && actions && values && n_steps >= 0 && eval_buffers_ok(b);
}

// ---- what the tile forms read off the env ---------------------------------------------------------------------------------------------
// ORCA agents / box scenarios generated inside the step: the env step's RVO instantiation (as cavoid_step_autoreset routes them)
inline bool loop_rvo_form(const cavoid_env *e) { return e->cfg.rvo_enabled || (e->cfg.gen_mode == 1 && e->pool_size <= 0); }

// the observation tile of a wavefront's env step, in floats (at least the parked rows)
inline int loop_tile_floats(const KCfg &k) {
    const int tile = (k.tile_rows * k.width + 3) & ~3;
    return tile < k.park_floats ? k.park_floats : tile;
}

inline unsigned loop_tile_count(const cavoid_env *e) { return (unsigned)((e->W + e->k.wpw - 1) / e->k.wpw); }

// The env's kernel configuration as a loop kernel takes it.  stream_obs = false: the tile's own policy phase reads the rows next, they
// stay in the L2 -- every tile form and every evaluation form.  stream_obs = true passes e->k as it is: the three crowd actor forms.
inline KCfg loop_kcfg(const cavoid_env *e, bool stream_obs) {
    KCfg k = e->k;
    if (!stream_obs) k.stream_obs = 0;
    return k;
}

// scenario look-ahead: the rings cover n_steps restarts, and the launch behind this consumes them (the actor forms and cavoid_step_push)
inline int loop_ahead_prepare(cavoid_env *e, int32_t n_steps, hipStream_t s) {
    if (int rc = cavoid_ahead_prepare(e, n_steps, s)) return rc;
    cavoid_ahead_consumed(e, n_steps);
    return CAVOID_OK;
}

// ---- kernel-argument fills ----------------------------------------------------------------------------------------------------------
// the policy pass inside a loop kernel, either network (x: the step's observation buffer, set by the kernel)
inline PolicyArgs loop_policy_args(const cavoid_env *e, const cavoid_policy *h) {
    PolicyArgs a = policy_common_args(h, nullptr, e->A, e->k.width);
    a.seed_lo = (uint32_t)h->seed; a.seed_hi = (uint32_t)(h->seed >> 32);
    a.step_counter = h->step_counter; a.blocks_done = h->blocks_done;
    return a;
}

inline SplitArgs split_args(const cavoid_env *e, const cavoid_policy *h) { return SplitArgs{loop_policy_args(e, h), h->sfrags, h->sbias}; }

// The frozen network of an rnn form (argmax only): the learner's arguments with the frozen handle's weights, biases and normalisation.
// It KEEPS the learner's seed, step and block counters and cu_tickets.
inline SplitArgs frozen_split_args(const SplitArgs &sa, const cavoid_policy *frozen) {
    SplitArgs fz = sa;
    fz.p.avg = frozen->normalize ? frozen->avg : nullptr; fz.p.std = frozen->normalize ? frozen->std : nullptr;
    fz.p.frags = frozen->frags; fz.p.bias = frozen->bias; fz.p.min_policy = frozen->min_policy;
    fz.sfrags = frozen->sfrags; fz.sbias = frozen->sbias;
    return fz;
}

// The frozen network of a weight-sharing form (argmax only): the frozen handle's own arguments.  It keeps NOTHING of the learner: zero
// seed, null step and block counters, the frozen handle's cu_tickets.
inline PolicyArgs frozen_ws_args(const cavoid_env *e, const cavoid_policy *frozen) { return policy_common_args(frozen, nullptr, e->A, e->k.width); }

inline RolloutCfg rollout_cfg(const cavoid_rollout *r, const cavoid_rollout_buffers *b) {
    RolloutCfg rc = r->c;
    rc.dup_capacity = b->dup_capacity; rc.ep_capacity = b->ep_capacity;
    return rc;
}

// step: the ring row of cavoid_step_push, -1 inside a loop (the device-side counter)
inline RolloutIO rollout_io(const cavoid_rollout_buffers *b, int32_t step) {
    RolloutIO rio{};
    rio.step = step; rio.x = b->x; rio.val = b->val; rio.ret = b->ret; rio.act = b->act; rio.emit_t = b->emit_t;
    rio.dup_x = b->dup_x; rio.dup_r = b->dup_r; rio.dup_a = b->dup_a; rio.dup_src = b->dup_src; rio.dup_count = b->dup_count;
    rio.ep_out = b->ep_out; rio.ep_count = b->ep_count;
    return rio;
}

// (quad stays 0: the tile forms set it from quad_form)
inline ActorIO actor_io(const cavoid_rollout *r, float *obs_cur, float *obs_next, float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions,
                        float *values, int32_t n_steps, int32_t greedy) {
    ActorIO io{};
    io.obs[0] = obs_cur; io.obs[1] = obs_next; io.rewards = rewards; io.done = done; io.game_over = game_over;
    io.actions = actions; io.values = values; io.rollout_step = r->s.step_counter; io.n_steps = n_steps; io.greedy = greedy ? 1 : 0;
    return io;
}

inline EvalIO eval_io(const cavoid_eval_buffers *b, float *obs, float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values,
                      int32_t n_steps, int32_t greedy) {
    EvalIO io{};
    io.obs = obs; io.rewards = rewards; io.done = done; io.game_over = game_over; io.actions = actions; io.values = values;
    io.ret = b->ret; io.goal_step = b->goal_step; io.world_steps = b->world_steps; io.worlds_running = b->worlds_running;
    io.n_steps = n_steps; io.greedy = greedy ? 1 : 0;
    return io;
}

// The tile's env step spread over the workgroup's four wavefronts (cavoid_quad.hpp) where that form carries the configuration: not the
// ORCA / in-step box instantiation, at most MAX_AGENTS_QUAD agents (kActorQuadMaxAgents / kEvalQuadMaxAgents: what the kernel instantiates),
// one pass per tile, its LDS inside the `lent` bytes.  CAVOID_ACTOR_QUAD=0: wavefront 0 alone (A/B runs).
template <int MAX_AGENTS_QUAD>
inline int quad_form(const cavoid_env *e, bool rvo_form, size_t lent) {
    const KCfg &k = e->k;
    int quad = (!rvo_form && e->cfg.max_agents <= MAX_AGENTS_QUAD && k.tile_rows >= k.wpw * e->cfg.max_agents &&
                quad_lds_bytes<MAX_AGENTS_QUAD>((k.tile_rows * k.width + 3) & ~3) <= lent) ? 1 : 0;
    if (const char *ov = std::getenv("CAVOID_ACTOR_QUAD")) quad = (quad && std::atoi(ov) != 0) ? 1 : 0;
    return quad;
}

// ---- the big-LDS launch -------------------------------------------------------------------------------------------------------------
// One 256-thread launch of Kernel with `lds` bytes of dynamic LDS above 64 KiB: opted into once per kernel instantiation AND device (the
// attribute belongs to the function on the current device; a process may drive several).  The flags are keyed on the kernel's address,
// not its type: two instantiations of one kernel template share a function-pointer type.  They are only ever set, and setting the
// attribute twice is harmless: no lock.
template <auto Kernel, class... Args>
static int launch_big_lds(int dev, size_t lds, unsigned tiles, hipStream_t s, const Args &...args) {
    static bool opted_in[64] = {};
    if (dev < 0 || dev >= 64 || !opted_in[dev]) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (dev >= 0 && dev < 64) opted_in[dev] = true;
    }
    hipLaunchKernelGGL(Kernel, dim3(tiles), dim3(256), lds, s, args...);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

// ---- the crowd launches' prologue and bucket ---------------------------------------------------------------------------------------------
// What every crowd loop launch refuses before it launches, in this order: an agent count the crowd form does not carry and -- where
// refuse_ahead -- a look-ahead env (CAVOID_EUNSUPPORTED); a tile count out of range (CAVOID_EINVAL); an env step whose LDS (crowd_kernel's
// allocation) does not fit 64 KiB or the `lent` bytes of the idle activation rows, so that what lies behind them survives it
// (CAVOID_EUNSUPPORTED).  refuse_ahead: true for the three actor forms and cavoid_crowd_eval_run_mix, false for cavoid_crowd_eval_run and
// cavoid_crowd_eval_run_ws.  lent: 2 * kSpPlaneB for the rnn forms, actor_ws_lent_bytes() for the weight-sharing forms.
inline int crowd_loop_tiles(const cavoid_env *e, size_t lent, bool refuse_ahead, unsigned *tiles) {
    const KCfg &k = e->k;
    const int n = e->cfg.max_agents;
    if (!crowd_form(n) || n < 2 || n > CAVOID_MAX_AGENTS || (refuse_ahead && k.ahead > 0)) return CAVOID_EUNSUPPORTED;
    const int64_t t = (e->W + k.wpw - 1) / k.wpw;
    if (t < 1 || t > 0x7fffffffLL) return CAVOID_EINVAL;
    const size_t lds = crowd_actor_env_lds_bytes(n, k.tile_rows, k.width);
    if (lds > 65536 || lds > lent) return CAVOID_EUNSUPPORTED;
    *tiles = (unsigned)t;
    return CAVOID_OK;
}

// f(std::integral_constant<int, NB>{}, std::bool_constant<RVO>{}) for a crowd kernel's instantiation: the bucket NB of the agent count
// (17..32, 33..64; N itself is a kernel argument) x the ORCA-carrying env step of an env whose worlds may hold ORCA agents
// (cfg.rvo_enabled = CAVOID_RVO_WAVE), as cavoid_launch_crowd_push routes
template <class F>
static inline int dispatch_crowd_bucket(int n, bool rvo, F &&f) {
    using NB32 = std::integral_constant<int, 32>;
    using NB64 = std::integral_constant<int, 64>;
    if (rvo) return n <= 32 ? f(NB32{}, std::true_type{}) : f(NB64{}, std::true_type{});
    return n <= 32 ? f(NB32{}, std::false_type{}) : f(NB64{}, std::false_type{});
}

}  // namespace cavoid
