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

template <int NB, bool RVO>
static int launch_crowd_mix_rollout(cavoid_env *e, unsigned tiles, const SplitArgs &sa, const SplitArgs &fz, const RolloutCfg &rc, const RolloutState &rs,
                                    const RolloutIO &rio, const ActorIO &io, hipStream_t s) {
    // > 64 KiB of dynamic LDS: opted into once per instantiation and device (see launch_actor)
    static bool opted_in[64] = {};
    const int dev = e->device;
    if (dev < 0 || dev >= 64 || !opted_in[dev]) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(crowd_mix_rollout_kernel<NB, RVO>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)policy_split_lds_bytes()));
        if (dev >= 0 && dev < 64) opted_in[dev] = true;
    }
    hipLaunchKernelGGL((crowd_mix_rollout_kernel<NB, RVO>), dim3(tiles), dim3(256), policy_split_lds_bytes(), s, e->k, e->st, (const PoolRec *)e->pool, sa, fz,
                       rc, rs, rio, io, e->cfg.max_agents);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

static int launch_crowd_mix_rollout_any(cavoid_env *e, const SplitArgs &sa, const SplitArgs &fz, const RolloutCfg &rc, const RolloutState &rs,
                                        const RolloutIO &rio, const ActorIO &io, hipStream_t s) {
    const KCfg &k = e->k;
    const int n = e->cfg.max_agents;
    if (!crowd_form(n) || n < 2 || n > CAVOID_MAX_AGENTS || k.ahead > 0) return CAVOID_EUNSUPPORTED;    // (cavoid_launch_crowd_actor's refusals)
    const int64_t tiles = (e->W + k.wpw - 1) / k.wpw;
    if (tiles < 1 || tiles > 0x7fffffffLL) return CAVOID_EINVAL;
    // the env step borrows the (idle) activation planes: crowd_kernel's allocation, at most 64 KB of the planes' 66 KB -- the live mask
    // behind the planes survives it (cavoid_launch_crowd_actor's check)
    const size_t lds = crowd_actor_env_lds_bytes(n, k.tile_rows, k.width);
    if (lds > 65536 || lds > (size_t)2 * kSpPlaneB) return CAVOID_EUNSUPPORTED;
    // an env whose worlds may hold ORCA agents (cfg.rvo_enabled = CAVOID_RVO_WAVE): the ORCA-carrying env step, as cavoid_launch_crowd_push routes
    if (k.rvo_enabled)
        return n <= 32 ? launch_crowd_mix_rollout<32, true>(e, (unsigned)tiles, sa, fz, rc, rs, rio, io, s)
                       : launch_crowd_mix_rollout<64, true>(e, (unsigned)tiles, sa, fz, rc, rs, rio, io, s);
    return n <= 32 ? launch_crowd_mix_rollout<32, false>(e, (unsigned)tiles, sa, fz, rc, rs, rio, io, s)
                   : launch_crowd_mix_rollout<64, false>(e, (unsigned)tiles, sa, fz, rc, rs, rio, io, s);
}

extern "C" int cavoid_crowd_actor_run_mix(cavoid_env *e, cavoid_policy *h, cavoid_policy *frozen, cavoid_rollout *r, const cavoid_rollout_buffers *b,
                                          float *obs_cur, float *obs_next, float *rewards, uint8_t *done, uint8_t *game_over, int32_t *actions,
                                          float *values, int32_t n_steps, int32_t greedy, void *stream) {
    if (!e || !h || !frozen || !r || !b || b->struct_size != (int32_t)sizeof(cavoid_rollout_buffers) || !obs_cur || !obs_next || obs_cur == obs_next ||
        !rewards || !done || !game_over || !actions || !values || n_steps < 0)
        return CAVOID_EINVAL;
    if (!b->x || !b->val || !b->ret || !b->act || !b->emit_t || !b->dup_x || !b->dup_r || !b->dup_a || !b->dup_src || !b->dup_count ||
        !b->ep_out || !b->ep_count || b->dup_capacity < 1 || b->ep_capacity < 1)
        return CAVOID_EINVAL;
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
    if (int rc_a = cavoid_ahead_prepare(e, n_steps, s)) return rc_a;      // (as cavoid_step_push; the crowd form has no scenario look-ahead)
    cavoid_ahead_consumed(e, n_steps);

    PolicyArgs a{};
    a.rows = e->A; a.stride = e->k.width; a.max_other = h->max_other; a.num_actions = h->num_actions; a.in_size = h->in_size;
    a.avg = h->normalize ? h->avg : nullptr; a.std = h->normalize ? h->std : nullptr;
    a.frags = h->frags; a.bias = h->bias; a.min_policy = h->min_policy;
    a.seed_lo = (uint32_t)h->seed; a.seed_hi = (uint32_t)(h->seed >> 32);
    a.step_counter = h->step_counter; a.blocks_done = h->blocks_done; a.cu_tickets = h->cu_tickets;
    const SplitArgs sa{a, h->sfrags, h->sbias};
    SplitArgs fz = sa;                                       // the frozen network: same shapes, its own weights / normalisation; argmax only
    fz.p.avg = frozen->normalize ? frozen->avg : nullptr; fz.p.std = frozen->normalize ? frozen->std : nullptr;
    fz.p.frags = frozen->frags; fz.p.bias = frozen->bias; fz.p.min_policy = frozen->min_policy;
    fz.sfrags = frozen->sfrags; fz.sbias = frozen->sbias;
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
    const int rc_launch = note_form(e, launch_crowd_mix_rollout_any(e, sa, fz, rc, r->s, rio, io, s), crowd_step_form(e));   // (reported as after cavoid_step_push)
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_actor_finish(r->s.step_counter, h->step_counter, n_steps, s);
}
