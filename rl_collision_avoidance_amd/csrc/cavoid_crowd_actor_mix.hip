// cavoid_crowd_actor_mix.hip -- C ABI (include/cavoid.h, cavoid_crowd_actor_run_mix) over crowd_mix_rollout_kernel<NB, RVO>
// (cavoid_crowd_actor_mix.hpp): cavoid_actor_run_mix on an env of more than kTileMaxAgents agents per world -- the closed loop of crowd worlds
// with a second, frozen network for the CAVOID_POLICY_FROZEN_NET agents, K steps in ONE launch.  Two buckets of the agent count (17..32, 33..64)
// x (plain, ORCA-carrying env step), as cavoid_crowd_actor.hip; N itself is a kernel argument.  Own translation unit, compiled with
// -mllvm -disable-machine-licm like every other step-loop unit (build.py).
#include "cavoid_actor_host.hpp"
#include "cavoid_crowd_actor_mix.hpp"
#include "cavoid_policy_host.hpp"
#include "cavoid_rollout_host.hpp"

using namespace cavoid;

static int launch_crowd_mix_rollout_any(cavoid_env *e, const SplitArgs &sa, const SplitArgs &fz, const RolloutCfg &rc, const RolloutState &rs,
                                        const RolloutIO &rio, const ActorIO &io, hipStream_t s) {
    // the env step borrows the (idle) activation planes: cavoid_launch_crowd_actor's bound
    unsigned tiles = 0;
    if (int rc_t = crowd_loop_tiles(e, /*lent=*/(size_t)2 * kSpPlaneB, /*refuse_ahead=*/true, &tiles)) return rc_t;
    return dispatch_crowd_bucket(e->cfg.max_agents, e->k.rvo_enabled != 0, [&](auto nb, auto rvo) {
        return launch_big_lds<crowd_mix_rollout_kernel<decltype(nb)::value, decltype(rvo)::value>>(
            e->device, policy_split_lds_bytes(), tiles, s, loop_kcfg(e, /*stream_obs=*/true), e->st, (const PoolRec *)e->pool, sa, fz, rc, rs, rio, io,
            e->cfg.max_agents);
    });
}

extern "C" int cavoid_crowd_actor_run_mix(cavoid_env *e, cavoid_policy *h, cavoid_policy *frozen, cavoid_rollout *r, const cavoid_rollout_buffers *b,
                                          float *obs_cur, float *obs_next, float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions,
                                          float *values, int32_t n_steps, int32_t greedy, void *stream) {
    if (!frozen || !actor_args_ok(e, h, r, b, obs_cur, obs_next, rewards, done, game_over, actions, values, n_steps)) return CAVOID_EINVAL;
    if (h->ws || frozen->ws) return CAVOID_EUNSUPPORTED;     // (the kernel embeds the LSTM pass, twice: a weight-sharing handle acts step by step)
    if (n_steps == 0) return CAVOID_OK;
    if (!h->loaded || !frozen->loaded) return CAVOID_EINVAL;
    // a neighbour count that is not the env's: no pass of this launch reads such rows
    if (h->max_other != e->cfg.max_other) return CAVOID_EUNSUPPORTED;
    // the handles must describe the same batch
    if (h->device != e->device || frozen->device != e->device || r->device != e->device || r->c.num_slots != e->A ||
        r->c.max_agents != e->cfg.max_agents || r->c.obs_width != e->k.width || h->in_size != e->k.width - 1)
        return CAVOID_EINVAL;
    // what the kernel does not carry -- what cavoid_crowd_actor_run refuses, for the same reasons; tile worlds have cavoid_actor_run_mix
    if (e->cfg.dynamics == CAVOID_DYN_HOLONOMIC || !h->use_split || h->split_products != kSpDefaultProducts) return CAVOID_EUNSUPPORTED;
    if (e->cfg.max_agents <= kTileMaxAgents) return CAVOID_EUNSUPPORTED;
    // the frozen network: the learner's shapes and the default inference form (cavoid_actor_run_mix's check)
    if (frozen->in_size != h->in_size || frozen->max_other != h->max_other || frozen->num_actions != h->num_actions || !frozen->use_split ||
        frozen->split_products != kSpDefaultProducts)
        return CAVOID_EUNSUPPORTED;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc_a = loop_ahead_prepare(e, n_steps, s)) return rc_a;        // (as cavoid_step_push; the crowd form has no scenario look-ahead)

    const SplitArgs sa = split_args(e, h);
    const SplitArgs fz = frozen_split_args(sa, frozen);     // same shapes, its own weights / normalisation; argmax only
    const RolloutCfg rc = rollout_cfg(r, b);
    const RolloutIO rio = rollout_io(b, -1);
    const ActorIO io = actor_io(r, obs_cur, obs_next, rewards, done, game_over, actions, values, n_steps, greedy);
    e->last_form = CAVOID_FORM_NONE;
    const int rc_launch = note_form(e, launch_crowd_mix_rollout_any(e, sa, fz, rc, r->s, rio, io, s), crowd_step_form(e));   // (reported as after cavoid_step_push)
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_actor_finish(r->s.step_counter, h->step_counter, n_steps, s);
}
