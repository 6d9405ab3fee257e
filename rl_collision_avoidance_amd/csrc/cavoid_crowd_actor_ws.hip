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

template <int NB, bool RVO>
static int launch_crowd_ws_rollout(cavoid_env *e, unsigned tiles, const PolicyWsArgs &wa, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio,
                                   const ActorIO &io, hipStream_t s) {
    // > 64 KiB of dynamic LDS: opted into once per instantiation and device (see launch_crowd_actor)
    static bool opted_in[64] = {};
    const int dev = e->device;
    if (dev < 0 || dev >= 64 || !opted_in[dev]) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(crowd_ws_rollout_kernel<NB, RVO>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)policy_lds_bytes(4)));
        if (dev >= 0 && dev < 64) opted_in[dev] = true;
    }
    hipLaunchKernelGGL((crowd_ws_rollout_kernel<NB, RVO>), dim3(tiles), dim3(256), policy_lds_bytes(4), s, e->k, e->st, (const PoolRec *)e->pool, wa, rc, rs,
                       rio, io, e->cfg.max_agents);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

static int launch_crowd_ws_rollout_any(cavoid_env *e, const PolicyWsArgs &wa, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio,
                                       const ActorIO &io, hipStream_t s) {
    const KCfg &k = e->k;
    const int n = e->cfg.max_agents;
    if (!crowd_form(n) || n < 2 || n > CAVOID_MAX_AGENTS || k.ahead > 0) return CAVOID_EUNSUPPORTED;    // (cavoid_launch_crowd_actor's refusals)
    const int64_t tiles = (e->W + k.wpw - 1) / k.wpw;
    if (tiles < 1 || tiles > 0x7fffffffLL) return CAVOID_EINVAL;
    // the env step borrows the (idle) activation rows: crowd_kernel's allocation, at most 64 KB of the rows' 65 KB -- the live mask and the
    // row list behind them survive it
    const size_t lds = crowd_actor_env_lds_bytes(n, k.tile_rows, k.width);
    if (lds > 65536 || lds > actor_ws_lent_bytes()) return CAVOID_EUNSUPPORTED;
    // an env whose worlds may hold ORCA agents (cfg.rvo_enabled = CAVOID_RVO_WAVE): the ORCA-carrying env step, as cavoid_launch_crowd_push routes
    if (k.rvo_enabled)
        return n <= 32 ? launch_crowd_ws_rollout<32, true>(e, (unsigned)tiles, wa, rc, rs, rio, io, s)
                       : launch_crowd_ws_rollout<64, true>(e, (unsigned)tiles, wa, rc, rs, rio, io, s);
    return n <= 32 ? launch_crowd_ws_rollout<32, false>(e, (unsigned)tiles, wa, rc, rs, rio, io, s)
                   : launch_crowd_ws_rollout<64, false>(e, (unsigned)tiles, wa, rc, rs, rio, io, s);
}

extern "C" int cavoid_crowd_actor_run_ws(cavoid_env *e, cavoid_policy *h, cavoid_rollout *r, const cavoid_rollout_buffers *b, float *obs_cur, float *obs_next,
                                         float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps,
                                         int32_t greedy, void *stream) {
    if (!e || !h || !r || !b || b->struct_size != (int32_t)sizeof(cavoid_rollout_buffers) || !obs_cur || !obs_next || obs_cur == obs_next ||
        !rewards || !done || !game_over || !actions || !values || n_steps < 0)
        return CAVOID_EINVAL;
    if (!b->x || !b->val || !b->ret || !b->act || !b->emit_t || !b->dup_x || !b->dup_r || !b->dup_a || !b->dup_src || !b->dup_count ||
        !b->ep_out || !b->ep_count || b->dup_capacity < 1 || b->ep_capacity < 1)
        return CAVOID_EINVAL;
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
    if (int rc_a = cavoid_ahead_prepare(e, n_steps, s)) return rc_a;      // (as cavoid_step_push; the crowd form has no scenario look-ahead)
    cavoid_ahead_consumed(e, n_steps);

    PolicyWsArgs wa{};
    wa.a = policy_common_args(h, nullptr, e->A, e->k.width);   // (x: the step's observation buffer, set by the kernel)
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
    e->last_form = CAVOID_FORM_NONE;
    const int rc_launch = note_form(e, launch_crowd_ws_rollout_any(e, wa, rc, r->s, rio, io, s), crowd_step_form(e));   // (reported as after cavoid_step_push)
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_actor_finish(r->s.step_counter, h->step_counter, n_steps, s);
}
