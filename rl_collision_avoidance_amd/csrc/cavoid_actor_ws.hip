// cavoid_actor_ws.hip -- C ABI (include/cavoid.h, cavoid_actor_run_ws) over actor_ws_kernel<N, RVO> (cavoid_actor_ws.hpp): K closed-loop
// GA3C actor steps of the weight-sharing network -- policy forward, action selection, env.step, experience bookkeeping -- in ONE launch.
// Own translation unit (the kernel carries the weight-sharing pass and the env step; instantiated per agent count).
#include <cstdlib>
#include "cavoid_actor_host.hpp"
#include "cavoid_actor_ws_host.hpp"
#include "cavoid_policy_host.hpp"
#include "cavoid_rollout_host.hpp"

using namespace cavoid;

extern "C" int cavoid_actor_run_ws(cavoid_env *e, cavoid_policy *h, cavoid_rollout *r, const cavoid_rollout_buffers *b, float *obs_cur, float *obs_next,
                                   float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps,
                                   int32_t greedy, void *stream) {
    if (!e || !h || !r || !b || b->struct_size != (int32_t)sizeof(cavoid_rollout_buffers) || !obs_cur || !obs_next || obs_cur == obs_next ||
        !rewards || !done || !game_over || !actions || !values || n_steps < 0)
        return CAVOID_EINVAL;
    if (!b->x || !b->val || !b->ret || !b->act || !b->emit_t || !b->dup_x || !b->dup_r || !b->dup_a || !b->dup_src || !b->dup_count ||
        !b->ep_out || !b->ep_count || b->dup_capacity < 1 || b->ep_capacity < 1)
        return CAVOID_EINVAL;
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
    const KCfg &k = e->k;
    // ORCA agents / box scenarios generated inside the step: the env step's RVO instantiation (as cavoid_step_autoreset routes them)
    const bool rvo_form = e->cfg.rvo_enabled || (e->cfg.gen_mode == 1 && e->pool_size <= 0);
    int tile = (k.tile_rows * k.width + 3) & ~3;
    if (tile < k.park_floats) tile = k.park_floats;
    // the env step borrows the (idle) activation rows: staging arrays + obs tile (+ the ORCA lines)
    if (actor_env_lds_bytes(e->cfg.max_agents, tile, k.rvo_lds_floats) > actor_ws_lent_bytes()) return CAVOID_EUNSUPPORTED;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc_a = cavoid_ahead_prepare(e, n_steps, s)) return rc_a;     // (scenario look-ahead: the rings cover n_steps restarts)
    cavoid_ahead_consumed(e, n_steps);

    PolicyWsArgs wa{};
    wa.a = policy_common_args(h, nullptr, e->A, k.width);   // (x: the step's observation buffer, set by the kernel)
    wa.a.seed_lo = (uint32_t)h->seed; wa.a.seed_hi = (uint32_t)(h->seed >> 32);
    wa.a.step_counter = h->step_counter; wa.a.blocks_done = h->blocks_done;
    RolloutCfg rc = r->c;
    rc.dup_capacity = b->dup_capacity; rc.ep_capacity = b->ep_capacity;
    RolloutIO rio{};
    rio.step = -1; rio.x = b->x; rio.val = b->val; rio.ret = b->ret; rio.act = b->act; rio.emit_t = b->emit_t;
    rio.dup_x = b->dup_x; rio.dup_r = b->dup_r; rio.dup_a = b->dup_a; rio.dup_src = b->dup_src; rio.dup_count = b->dup_count;
    rio.ep_out = b->ep_out; rio.ep_count = b->ep_count;
    ActorIO io{};
    io.obs[0] = obs_cur; io.obs[1] = obs_next; io.rewards = rewards; io.done = done; io.game_over = game_over;
    io.actions = actions; io.values = values; io.rollout_step = r->s.step_counter; io.n_steps = n_steps; io.greedy = greedy ? 1 : 0;
    // the tile's env step spread over the workgroup's four wavefronts (cavoid_quad.hpp) where that form carries the configuration, as
    // cavoid_actor_run decides it -- its LDS inside the lent rows (CAVOID_ACTOR_QUAD=0: wavefront 0 alone, A/B runs)
    io.quad = (!rvo_form && e->cfg.max_agents <= kActorQuadMaxAgents && k.tile_rows >= k.wpw * e->cfg.max_agents &&
               quad_lds_bytes<kActorQuadMaxAgents>((k.tile_rows * k.width + 3) & ~3) <= actor_ws_lent_bytes()) ? 1 : 0;
    if (const char *ov = std::getenv("CAVOID_ACTOR_QUAD")) io.quad = (io.quad && std::atoi(ov) != 0) ? 1 : 0;
    const int rc_launch = rvo_form ? cavoid_launch_actor_ws_rvo(e, wa, rc, r->s, rio, io, s) : launch_actor_ws_any<false>(e, wa, rc, r->s, rio, io, s);
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_actor_finish(r->s.step_counter, h->step_counter, n_steps, s);
}
