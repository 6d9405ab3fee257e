// cavoid_actor_ws.hip -- C ABI (include/cavoid.h, cavoid_actor_run_ws) over actor_ws_kernel<N, RVO> (cavoid_actor_ws.hpp): K closed-loop
// GA3C actor steps of the weight-sharing network -- policy forward, action selection, env.step, experience bookkeeping -- in ONE launch.
// Own translation unit (the kernel carries the weight-sharing pass and the env step; instantiated per agent count).
#include "cavoid_actor_host.hpp"
#include "cavoid_actor_ws_host.hpp"
#include "cavoid_policy_host.hpp"
#include "cavoid_rollout_host.hpp"

using namespace cavoid;

extern "C" int cavoid_actor_run_ws(cavoid_env *e, cavoid_policy *h, cavoid_rollout *r, const cavoid_rollout_buffers *b, float *obs_cur, float *obs_next,
                                   float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps,
                                   int32_t greedy, void *stream) {
    if (!actor_args_ok(e, h, r, b, obs_cur, obs_next, rewards, done, game_over, actions, values, n_steps)) return CAVOID_EINVAL;
    // the kernel embeds the weight-sharing pass on the whole parked row: an LSTM handle has cavoid_actor_run, a ring handle
    // (cavoid_policy_create_ws_crowd, 20..64 neighbours) acts step by step
    if (!h->ws || h->crowd || h->max_other > kWsMaxOthers) return CAVOID_EUNSUPPORTED;
    if (n_steps == 0) return CAVOID_OK;
    if (!h->loaded) return CAVOID_EINVAL;
    // the three handles must describe the same batch
    if (h->device != e->device || r->device != e->device || r->c.num_slots != e->A || r->c.max_agents != e->cfg.max_agents ||
        r->c.obs_width != e->k.width || h->in_size != e->k.width - 1 || h->max_other != e->cfg.max_other)
        return CAVOID_EINVAL;
    // what the kernel does not carry (the step-by-step entry points do): crowd worlds, velocity actions
    if (e->cfg.max_agents > kTileMaxAgents) return CAVOID_EUNSUPPORTED;
    if (e->cfg.dynamics == CAVOID_DYN_HOLONOMIC) return CAVOID_EUNSUPPORTED;
    // frozen-network agents act by THEIR network, and this launch carries one (no _mix form): an env whose generator makes them acts step by step
    if (e->cfg.gen_frozen_fraction > 0.0 && e->cfg.gen_nonlearning_fraction > 0.0) return CAVOID_EUNSUPPORTED;
    // the env step borrows the (idle) activation rows: staging arrays + obs tile (+ the ORCA lines)
    const size_t lent = actor_ws_lent_bytes();
    if (actor_env_lds_bytes(e->cfg.max_agents, loop_tile_floats(e->k), e->k.rvo_lds_floats) > lent) return CAVOID_EUNSUPPORTED;
    const bool rvo_form = loop_rvo_form(e);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc_a = loop_ahead_prepare(e, n_steps, s)) return rc_a;

    PolicyWsArgs wa{};
    wa.a = loop_policy_args(e, h);
    const RolloutCfg rc = rollout_cfg(r, b);
    const RolloutIO rio = rollout_io(b, -1);
    ActorIO io = actor_io(r, obs_cur, obs_next, rewards, done, game_over, actions, values, n_steps, greedy);
    io.quad = quad_form<kActorQuadMaxAgents>(e, rvo_form, lent);      // (as cavoid_actor_run decides it, inside the lent rows)
    const int rc_launch = rvo_form ? cavoid_launch_actor_ws_rvo(e, wa, rc, r->s, rio, io, s) : launch_actor_ws_any<false>(e, wa, rc, r->s, rio, io, s);
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_actor_finish(r->s.step_counter, h->step_counter, n_steps, s);
}
