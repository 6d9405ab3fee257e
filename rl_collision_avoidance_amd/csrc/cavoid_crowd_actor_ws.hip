// cavoid_crowd_actor_ws.hip -- C ABI (include/cavoid.h, cavoid_crowd_actor_run_ws) over crowd_ws_rollout_kernel<NB, RVO>
// (cavoid_crowd_actor_ws.hpp): K closed-loop GA3C actor steps of crowd worlds (17..64 agents) with the weight-sharing network -- the ring form of
// the weight-sharing pass on the tile's live rows, action selection, the crowd env step, experience bookkeeping -- in ONE launch.  Two buckets
// of the agent count (17..32, 33..64) x (plain, ORCA-carrying env step), as cavoid_crowd_actor.hip; N itself is a kernel argument, and the one
// ring instantiation of the pass serves every neighbour count 1..64.  Own translation unit, compiled with -mllvm -disable-machine-licm like
// every other step-loop unit (build.py).
#include "cavoid_actor_host.hpp"
#include "cavoid_crowd_actor_ws.hpp"
#include "cavoid_policy_host.hpp"
#include "cavoid_rollout_host.hpp"

using namespace cavoid;

static int launch_crowd_ws_rollout_any(cavoid_env *e, const PolicyWsArgs &wa, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio,
                                       const ActorIO &io, hipStream_t s) {
    // the env step borrows the (idle) activation rows: crowd_kernel's allocation, at most 64 KB of the rows' 65 KB -- the live mask and the
    // row list behind them survive it
    unsigned tiles = 0;
    if (int rc_t = crowd_loop_tiles(e, /*lent=*/actor_ws_lent_bytes(), /*refuse_ahead=*/true, &tiles)) return rc_t;
    return dispatch_crowd_bucket(e->cfg.max_agents, e->k.rvo_enabled != 0, [&](auto nb, auto rvo) {
        return launch_big_lds<crowd_ws_rollout_kernel<decltype(nb)::value, decltype(rvo)::value>>(
            e->device, policy_lds_bytes(4), tiles, s, loop_kcfg(e, /*stream_obs=*/true), e->st, (const PoolRec *)e->pool, wa, rc, rs, rio, io, e->cfg.max_agents);
    });
}

extern "C" int cavoid_crowd_actor_run_ws(cavoid_env *e, cavoid_policy *h, cavoid_rollout *r, const cavoid_rollout_buffers *b, float *obs_cur, float *obs_next,
                                         float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps,
                                         int32_t greedy, void *stream) {
    if (!actor_args_ok(e, h, r, b, obs_cur, obs_next, rewards, done, game_over, actions, values, n_steps)) return CAVOID_EINVAL;
    // the kernel embeds the weight-sharing pass in its ring form, which serves a cavoid_policy_create_ws handle (1..19 neighbours) and a
    // cavoid_policy_create_ws_crowd handle (20..64) alike: an LSTM handle has cavoid_crowd_actor_run
    if (!h->ws || h->max_other > kWsMaxOthersCrowd) return CAVOID_EUNSUPPORTED;
    if (n_steps == 0) return CAVOID_OK;
    if (!h->loaded) return CAVOID_EINVAL;
    // the three handles must describe the same batch
    if (h->device != e->device || r->device != e->device || r->c.num_slots != e->A || r->c.max_agents != e->cfg.max_agents ||
        r->c.obs_width != e->k.width || h->in_size != e->k.width - 1 || h->max_other != e->cfg.max_other)
        return CAVOID_EINVAL;
    // what the kernel does not carry (the step-by-step entry points do): tile worlds (cavoid_actor_run_ws carries those), velocity actions
    if (e->cfg.max_agents <= kTileMaxAgents) return CAVOID_EUNSUPPORTED;
    if (e->cfg.dynamics == CAVOID_DYN_HOLONOMIC) return CAVOID_EUNSUPPORTED;
    // frozen-network agents act by THEIR network, and this launch carries one (no _mix form): an env whose generator makes them acts step by step
    if (e->cfg.gen_frozen_fraction > 0.0 && e->cfg.gen_nonlearning_fraction > 0.0) return CAVOID_EUNSUPPORTED;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc_a = loop_ahead_prepare(e, n_steps, s)) return rc_a;        // (as cavoid_step_push; the crowd form has no scenario look-ahead)

    PolicyWsArgs wa{};
    wa.a = loop_policy_args(e, h);
    const RolloutCfg rc = rollout_cfg(r, b);
    const RolloutIO rio = rollout_io(b, -1);
    const ActorIO io = actor_io(r, obs_cur, obs_next, rewards, done, game_over, actions, values, n_steps, greedy);
    e->last_form = CAVOID_FORM_NONE;
    const int rc_launch = note_form(e, launch_crowd_ws_rollout_any(e, wa, rc, r->s, rio, io, s), crowd_step_form(e));   // (reported as after cavoid_step_push)
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_actor_finish(r->s.step_counter, h->step_counter, n_steps, s);
}
