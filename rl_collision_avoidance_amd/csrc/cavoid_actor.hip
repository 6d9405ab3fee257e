// cavoid_actor.hip -- C ABI (include/cavoid.h, cavoid_actor_run) over actor_kernel<N> (cavoid_actor.hpp): K closed-loop GA3C actor
// steps -- policy forward, action selection, env.step, experience bookkeeping -- in ONE launch.  Own translation unit (the
// kernel carries the policy's GEMM loops and the env step; instantiated per agent count).
#define CAVOID_ACTOR_KERNELS
#include "cavoid_actor_host.hpp"
#include "cavoid_policy_host.hpp"
#include "cavoid_rollout_host.hpp"

using namespace cavoid;

// actor_finish_kernel for the actor launches of this and of other translation units (cavoid_actor_ws.hip)
int cavoid_launch_actor_finish(int32_t *rollout_step, int32_t *policy_step, int32_t n_steps, hipStream_t s) {
    hipLaunchKernelGGL(actor_finish_kernel, dim3(1), dim3(1), 0, s, rollout_step, policy_step, n_steps);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

static int actor_run(cavoid_env *e, cavoid_policy *h, cavoid_policy *frozen, cavoid_rollout *r, const cavoid_rollout_buffers *b, float *obs_cur, float *obs_next,
                     float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps,
                     int32_t greedy, void *stream) {
    if (!actor_args_ok(e, h, r, b, obs_cur, obs_next, rewards, done, game_over, actions, values, n_steps)) return CAVOID_EINVAL;
    // the actor kernel embeds the LSTM pass: a weight-sharing handle (cavoid_policy_create_ws) acts step by step
    if (h->ws || (frozen && frozen->ws)) return CAVOID_EUNSUPPORTED;
    if (n_steps == 0) return CAVOID_OK;
    if (!h->loaded) return CAVOID_EINVAL;
    // the three handles must describe the same batch
    if (h->device != e->device || r->device != e->device || r->c.num_slots != e->A || r->c.max_agents != e->cfg.max_agents ||
        r->c.obs_width != e->k.width || h->in_size != e->k.width - 1 || h->max_other != e->cfg.max_other)
        return CAVOID_EINVAL;
    // what the fused kernel does not carry (the step-by-step entry points do): velocity actions, the float32-MFMA inference kernel
    // or a non-default number of split products (the kernel carries the default form of cavoid_policy_forward, so that both stay
    // bit-identical); frozen-network agents need a second network (BatchedRollout keeps those on the step-by-step path)
    if (e->cfg.dynamics == CAVOID_DYN_HOLONOMIC || !h->use_split || h->split_products != kSpDefaultProducts) return CAVOID_EUNSUPPORTED;
    if (e->cfg.max_agents > kTileMaxAgents) return CAVOID_EUNSUPPORTED;   // (the crowd form has no fused actor: env step + cavoid_rollout_push)
    // the actor kernel parks the whole input row (kPolMaxOthers): a crowd policy handle, M > 19 (an env of <= 16 agents padded wider), runs step by step
    if (h->max_other > kPolMaxOthers || (frozen && frozen->max_other > kPolMaxOthers)) return CAVOID_EUNSUPPORTED;
    // frozen-network agents act by THEIR network: without it this entry point would hand them the learner's sample
    if (!frozen && e->cfg.gen_frozen_fraction > 0.0 && e->cfg.gen_nonlearning_fraction > 0.0) return CAVOID_EUNSUPPORTED;
    if (frozen && (!frozen->loaded || frozen->device != e->device || frozen->in_size != h->in_size || frozen->max_other != h->max_other ||
                   frozen->num_actions != h->num_actions || !frozen->use_split || frozen->split_products != kSpDefaultProducts))
        return frozen->loaded ? CAVOID_EUNSUPPORTED : CAVOID_EINVAL;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc_a = loop_ahead_prepare(e, n_steps, s)) return rc_a;
    // the env step borrows the (idle) activation planes: staging arrays + obs tile (+ the ORCA lines, 64 (N-1) x 16 floats: N <= 12)
    const size_t lent = (size_t)2 * kSpPlaneB;
    if (actor_env_lds_bytes(e->cfg.max_agents, loop_tile_floats(e->k), e->k.rvo_lds_floats) > lent) return CAVOID_EUNSUPPORTED;
    const bool rvo_form = loop_rvo_form(e);

    const SplitArgs sa = split_args(e, h);
    const RolloutCfg rc = rollout_cfg(r, b);
    const RolloutIO rio = rollout_io(b, -1);
    ActorIO io = actor_io(r, obs_cur, obs_next, rewards, done, game_over, actions, values, n_steps, greedy);
    io.quad = quad_form<kActorQuadMaxAgents>(e, rvo_form, lent);
    const int rc_launch = frozen ? cavoid_launch_actor_frozen(e, sa, frozen_split_args(sa, frozen), rc, r->s, rio, io, s)
                                 : (rvo_form ? cavoid_launch_actor_rvo(e, sa, rc, r->s, rio, io, s) : launch_actor_any<false>(e, sa, sa, rc, r->s, rio, io, s));
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_actor_finish(r->s.step_counter, h->step_counter, n_steps, s);
}

extern "C" int cavoid_actor_run(cavoid_env *e, cavoid_policy *h, cavoid_rollout *r, const cavoid_rollout_buffers *b, float *obs_cur, float *obs_next,
                                float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps,
                                int32_t greedy, void *stream) {
    return actor_run(e, h, nullptr, r, b, obs_cur, obs_next, rewards, done, game_over, actions, values, n_steps, greedy, stream);
}

extern "C" int cavoid_actor_run_mix(cavoid_env *e, cavoid_policy *h, cavoid_policy *frozen, cavoid_rollout *r, const cavoid_rollout_buffers *b,
                                    float *obs_cur, float *obs_next, float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions,
                                    float *values, int32_t n_steps, int32_t greedy, void *stream) {
    if (!frozen) return CAVOID_EINVAL;
    return actor_run(e, h, frozen, r, b, obs_cur, obs_next, rewards, done, game_over, actions, values, n_steps, greedy, stream);
}

// cavoid_actor_run for crowd worlds (17..64 agents per world): crowd_actor_kernel<NB, RVO> (cavoid_crowd_actor.hpp, launched by
// cavoid_crowd_actor.hip) -- the ring form of the policy pass, the crowd env step and its bookkeeping per tile, K steps in one launch
extern "C" int cavoid_crowd_actor_run(cavoid_env *e, cavoid_policy *h, cavoid_rollout *r, const cavoid_rollout_buffers *b, float *obs_cur, float *obs_next,
                                      float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps,
                                      int32_t greedy, void *stream) {
    if (!actor_args_ok(e, h, r, b, obs_cur, obs_next, rewards, done, game_over, actions, values, n_steps)) return CAVOID_EINVAL;
    if (h->ws) return CAVOID_EUNSUPPORTED;                   // (the kernel embeds the LSTM pass: a weight-sharing handle acts step by step)
    if (n_steps == 0) return CAVOID_OK;
    if (!h->loaded) return CAVOID_EINVAL;
    // the three handles must describe the same batch
    if (h->device != e->device || r->device != e->device || r->c.num_slots != e->A || r->c.max_agents != e->cfg.max_agents ||
        r->c.obs_width != e->k.width || h->in_size != e->k.width - 1 || h->max_other != e->cfg.max_other)
        return CAVOID_EINVAL;
    // what the kernel does not carry (the step-by-step entry points do): velocity actions, the float32-MFMA inference kernel or the bf16
    // product form (it carries the default form of cavoid_policy_forward, so that both stay bit-identical); tile worlds have cavoid_actor_run
    if (e->cfg.dynamics == CAVOID_DYN_HOLONOMIC || !h->use_split || h->split_products != kSpDefaultProducts) return CAVOID_EUNSUPPORTED;
    if (e->cfg.max_agents <= kTileMaxAgents) return CAVOID_EUNSUPPORTED;
    // frozen-network agents act by THEIR network, and this launch carries one (no _mix form): an env whose generator makes them acts step by step
    if (e->cfg.gen_frozen_fraction > 0.0 && e->cfg.gen_nonlearning_fraction > 0.0) return CAVOID_EUNSUPPORTED;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc_a = loop_ahead_prepare(e, n_steps, s)) return rc_a;        // (as cavoid_step_push; the crowd form has no scenario look-ahead)

    const ActorIO io = actor_io(r, obs_cur, obs_next, rewards, done, game_over, actions, values, n_steps, greedy);
    e->last_form = CAVOID_FORM_NONE;
    const int rc_launch = note_form(e, cavoid_launch_crowd_actor(e, split_args(e, h), rollout_cfg(r, b), r->s, rollout_io(b, -1), io, s),
                                    crowd_step_form(e));     // (reported as after cavoid_step_push)
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_actor_finish(r->s.step_counter, h->step_counter, n_steps, s);
}

extern "C" int cavoid_step_push(cavoid_env *e, cavoid_rollout *r, const cavoid_rollout_buffers *b, const float *obs_cur, float *obs_next,
                                const int32_t *actions, const float *values, float *rewards, uint8_t *done, uint8_t *game_over, int32_t step,
                                void *stream) {
    if (!e || !r || !rollout_buffers_ok(b) || !obs_cur || !obs_next || obs_cur == obs_next || !actions || !values || !rewards || !done || !game_over)
        return CAVOID_EINVAL;
    if (r->device != e->device || r->c.num_slots != e->A || r->c.max_agents != e->cfg.max_agents || r->c.obs_width != e->k.width) return CAVOID_EINVAL;
    if (e->cfg.dynamics == CAVOID_DYN_HOLONOMIC) return CAVOID_EUNSUPPORTED;       // (velocity actions: cavoid_step_continuous + cavoid_rollout_push)
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc_a = loop_ahead_prepare(e, 1, s)) return rc_a;
    const RolloutCfg rc = rollout_cfg(r, b);
    const RolloutIO rio = rollout_io(b, step);
    // (one step on the caller's actions and values, which the kernel only reads; nothing is drawn: greedy stays 0)
    const ActorIO io = actor_io(r, const_cast<float *>(obs_cur), obs_next, rewards, done, game_over, const_cast<int32_t *>(actions), const_cast<float *>(values), 1, 0);
    const bool rvo_form = loop_rvo_form(e);
    int rc_launch;
    if (e->cfg.max_agents > kTileMaxAgents) {                // more than kTileMaxAgents agents per world: the crowd form's kernel (cavoid_crowd_push.hpp)
        e->last_form = CAVOID_FORM_NONE;
        rc_launch = note_form(e, cavoid_launch_crowd_push(e, rc, r->s, rio, io, step, s), crowd_step_form(e));
    } else {
        rc_launch = rvo_form ? cavoid_launch_step_push_rvo(e, rc, r->s, rio, io, step, s) : launch_step_push_any<false>(e, rc, r->s, rio, io, step, s);
    }
    if (rc_launch != CAVOID_OK) return rc_launch;
    if (step < 0) return cavoid_launch_actor_finish(r->s.step_counter, nullptr, 1, s);     // the device-side step counter moves on (hipGraph replays)
    return CAVOID_OK;
}

#ifdef CAVOID_TRACE
// development build only: the phase stamps of actor_kernel<N, false, false> (this translation unit's copy of g_pol_trace; tools/trace_actor.py)
extern "C" int cavoid_actor_debug_trace(unsigned long long *dev_ptr) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(cavoid::g_pol_trace), &dev_ptr, sizeof(dev_ptr)));
    return CAVOID_OK;
}
#endif
