// cavoid_crowd_eval_mix.hip -- C ABI (include/cavoid.h, cavoid_crowd_eval_run_mix) over crowd_mix_evaluate_kernel<NB, RVO>
// (cavoid_crowd_eval_mix.hpp): cavoid_eval_run with a `frozen` handle for an env of more than kTileMaxAgents agents per world.  Two buckets of the
// agent count (17..32, 33..64) x (plain, ORCA-carrying env step), as cavoid_crowd_eval.hip; N itself is a kernel argument.  Own translation unit,
// compiled with -mllvm -disable-machine-licm like every other step-loop unit (build.py).
#include "cavoid_crowd_eval_mix.hpp"
#include "cavoid_eval_host.hpp"
#include "cavoid_policy_host.hpp"

using namespace cavoid;

template <int NB, bool RVO>
static int launch_crowd_mix_eval(cavoid_env *e, unsigned tiles, const SplitArgs &sa, const SplitArgs &fz, const EvalIO &io, hipStream_t s) {
    // > 64 KiB of dynamic LDS: opted into once per instantiation and device (see launch_actor)
    static bool opted_in[64] = {};
    const int dev = e->device;
    if (dev < 0 || dev >= 64 || !opted_in[dev]) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(crowd_mix_evaluate_kernel<NB, RVO>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)eval_lds_bytes()));
        if (dev >= 0 && dev < 64) opted_in[dev] = true;
    }
    KCfg k = e->k;
    k.stream_obs = 0;                                        // (the tile's own policy phase reads the rows next: they stay in the L2)
    hipLaunchKernelGGL((crowd_mix_evaluate_kernel<NB, RVO>), dim3(tiles), dim3(256), eval_lds_bytes(), s, k, e->st, (const PoolRec *)e->pool, sa, fz, io,
                       e->cfg.max_agents);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

static int launch_crowd_mix_eval_any(cavoid_env *e, const SplitArgs &sa, const SplitArgs &fz, const EvalIO &io, hipStream_t s) {
    const KCfg &k = e->k;
    const int n = e->cfg.max_agents;
    if (!crowd_form(n) || n < 2 || n > CAVOID_MAX_AGENTS || k.ahead > 0) return CAVOID_EUNSUPPORTED;
    const int64_t tiles = (e->W + k.wpw - 1) / k.wpw;
    if (tiles < 1 || tiles > 0x7fffffffLL) return CAVOID_EINVAL;
    // the env step borrows the (idle) activation planes: crowd_kernel's allocation, what cavoid_launch_crowd_actor allows
    const size_t lds = crowd_actor_env_lds_bytes(n, k.tile_rows, k.width);
    if (lds > 65536 || lds > (size_t)2 * kSpPlaneB) return CAVOID_EUNSUPPORTED;
    // every tile ADDS its running worlds on leaving: the word starts from zero, on the stream
    HIP_TRY(hipMemsetAsync(io.worlds_running, 0, sizeof(int32_t), s));
    // an env whose worlds may hold ORCA agents (cfg.rvo_enabled = CAVOID_RVO_WAVE): the ORCA-carrying env step, as cavoid_launch_crowd routes
    if (k.rvo_enabled)
        return n <= 32 ? launch_crowd_mix_eval<32, true>(e, (unsigned)tiles, sa, fz, io, s) : launch_crowd_mix_eval<64, true>(e, (unsigned)tiles, sa, fz, io, s);
    return n <= 32 ? launch_crowd_mix_eval<32, false>(e, (unsigned)tiles, sa, fz, io, s) : launch_crowd_mix_eval<64, false>(e, (unsigned)tiles, sa, fz, io, s);
}

extern "C" int cavoid_crowd_eval_run_mix(cavoid_env *e, cavoid_policy *h, cavoid_policy *frozen, const cavoid_eval_buffers *b, float *obs, float *rewards,
                                         uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps, int32_t greedy,
                                         void *stream) {
    if (!e || !h || !frozen || !b || b->struct_size != (int32_t)sizeof(cavoid_eval_buffers) || !obs || !rewards || !done || !game_over || !actions ||
        !values || n_steps < 0)
        return CAVOID_EINVAL;
    if (!b->ret || !b->goal_step || !b->world_steps || !b->worlds_running) return CAVOID_EINVAL;
    if (h->ws || frozen->ws) return CAVOID_EUNSUPPORTED;     // (the kernel embeds the LSTM pass, twice: a weight-sharing handle evaluates step by step)
    if (n_steps == 0) return CAVOID_OK;
    if (!h->loaded || !frozen->loaded) return CAVOID_EINVAL;
    // a neighbour count that is not the env's: no pass of this launch reads such rows
    if (h->max_other != e->cfg.max_other) return CAVOID_EUNSUPPORTED;
    // the handles must describe the same batch
    if (h->device != e->device || frozen->device != e->device || h->in_size != e->k.width - 1) return CAVOID_EINVAL;
    // what the kernel does not carry -- what cavoid_crowd_eval_run refuses, for the same reasons; tile worlds have cavoid_eval_run
    if (e->cfg.dynamics == CAVOID_DYN_HOLONOMIC || !h->use_split || h->split_products != kSpDefaultProducts) return CAVOID_EUNSUPPORTED;
    if (e->cfg.max_agents <= kTileMaxAgents) return CAVOID_EUNSUPPORTED;
    // the frozen network: the learner's shapes and the default inference form (cavoid_eval_run's check)
    if (frozen->in_size != h->in_size || frozen->max_other != h->max_other || frozen->num_actions != h->num_actions || !frozen->use_split ||
        frozen->split_products != kSpDefaultProducts)
        return CAVOID_EUNSUPPORTED;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (no cavoid_ahead_prepare: nothing restarts)

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
    EvalIO io{};
    io.obs = obs; io.rewards = rewards; io.done = done; io.game_over = game_over; io.actions = actions; io.values = values;
    io.ret = b->ret; io.goal_step = b->goal_step; io.world_steps = b->world_steps; io.worlds_running = b->worlds_running;
    io.n_steps = n_steps; io.greedy = greedy ? 1 : 0;
    e->last_form = CAVOID_FORM_NONE;
    const int rc_launch = note_form(e, launch_crowd_mix_eval_any(e, sa, fz, io, s), crowd_step_form(e));     // (reported as after cavoid_step)
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_eval_finish(h->step_counter, n_steps, s);
}
