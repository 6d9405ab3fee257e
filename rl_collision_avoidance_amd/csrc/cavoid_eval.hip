// cavoid_eval.hip -- C ABI (include/cavoid.h, cavoid_eval_run) over eval_kernel<N> (cavoid_eval.hpp): K evaluation steps -- policy forward,
// action selection, env.step without auto-reset, outcome record -- in ONE launch that finished tiles leave early.  Own translation unit (the
// kernel carries the policy's GEMM loops and the env step; instantiated per agent count).
#include <cstdlib>
#define CAVOID_EVAL_KERNELS
#include "cavoid_eval_host.hpp"
#include "cavoid_policy_host.hpp"

using namespace cavoid;

extern "C" int cavoid_eval_run(cavoid_env *e, cavoid_policy *h, cavoid_policy *frozen, const cavoid_eval_buffers *b, float *obs, float *rewards,
                               uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps, int32_t greedy, void *stream) {
    if (!e || !h || !b || b->struct_size != (int32_t)sizeof(cavoid_eval_buffers) || !obs || !rewards || !done || !game_over || !actions || !values ||
        n_steps < 0)
        return CAVOID_EINVAL;
    if (!b->ret || !b->goal_step || !b->world_steps || !b->worlds_running) return CAVOID_EINVAL;
    // the kernel embeds the LSTM pass: a weight-sharing handle (cavoid_policy_create_ws) evaluates step by step
    if (h->ws || (frozen && frozen->ws)) return CAVOID_EUNSUPPORTED;
    if (n_steps == 0) return CAVOID_OK;
    if (!h->loaded) return CAVOID_EINVAL;
    // the handles must describe the same batch
    if (h->device != e->device || h->in_size != e->k.width - 1 || h->max_other != e->cfg.max_other) return CAVOID_EINVAL;
    // what the kernel does not carry -- exactly what cavoid_actor_run / _run_mix refuse (cavoid_actor.hip), for the same reasons
    if (e->cfg.dynamics == CAVOID_DYN_HOLONOMIC || !h->use_split || h->split_products != kSpDefaultProducts) return CAVOID_EUNSUPPORTED;
    if (e->cfg.max_agents > kTileMaxAgents) return CAVOID_EUNSUPPORTED;
    if (h->max_other > kPolMaxOthers || (frozen && frozen->max_other > kPolMaxOthers)) return CAVOID_EUNSUPPORTED;
    // frozen-network agents act by THEIR network: without it this entry point would hand them the learner's choice
    if (!frozen && e->cfg.gen_frozen_fraction > 0.0 && e->cfg.gen_nonlearning_fraction > 0.0) return CAVOID_EUNSUPPORTED;
    if (frozen && (!frozen->loaded || frozen->device != e->device || frozen->in_size != h->in_size || frozen->max_other != h->max_other ||
                   frozen->num_actions != h->num_actions || !frozen->use_split || frozen->split_products != kSpDefaultProducts))
        return frozen->loaded ? CAVOID_EUNSUPPORTED : CAVOID_EINVAL;
    HIP_TRY(hipSetDevice(e->device));
    // (no cavoid_ahead_prepare: nothing restarts)
    const KCfg &k = e->k;
    const bool rvo_form = e->cfg.rvo_enabled || (e->cfg.gen_mode == 1 && e->pool_size <= 0);      // actor_run's routing
    int tile = (k.tile_rows * k.width + 3) & ~3;
    if (tile < k.park_floats) tile = k.park_floats;
    // the env step borrows the (idle) activation planes: staging arrays + obs tile (+ the ORCA lines)
    if (eval_env_lds_bytes(e->cfg.max_agents, tile, k.rvo_lds_floats) > (size_t)2 * kSpPlaneB) return CAVOID_EUNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);

    PolicyArgs a{};
    a.rows = e->A; a.stride = k.width; a.max_other = h->max_other; a.num_actions = h->num_actions; a.in_size = h->in_size;
    a.avg = h->normalize ? h->avg : nullptr; a.std = h->normalize ? h->std : nullptr;
    a.frags = h->frags; a.bias = h->bias; a.min_policy = h->min_policy;
    a.seed_lo = (uint32_t)h->seed; a.seed_hi = (uint32_t)(h->seed >> 32);
    a.step_counter = h->step_counter; a.blocks_done = h->blocks_done; a.cu_tickets = h->cu_tickets;
    const SplitArgs sa{a, h->sfrags, h->sbias};
    SplitArgs fz = sa;                                       // the frozen network: same shapes, its own weights / normalisation; argmax only
    if (frozen) {
        fz.p.avg = frozen->normalize ? frozen->avg : nullptr; fz.p.std = frozen->normalize ? frozen->std : nullptr;
        fz.p.frags = frozen->frags; fz.p.bias = frozen->bias; fz.p.min_policy = frozen->min_policy;
        fz.sfrags = frozen->sfrags; fz.sbias = frozen->sbias;
    }
    EvalIO io{};
    io.obs = obs; io.rewards = rewards; io.done = done; io.game_over = game_over; io.actions = actions; io.values = values;
    io.ret = b->ret; io.goal_step = b->goal_step; io.world_steps = b->world_steps; io.worlds_running = b->worlds_running;
    io.n_steps = n_steps; io.greedy = greedy ? 1 : 0;
    // the tile's env step over the workgroup's four wavefronts where actor_run takes that form (CAVOID_ACTOR_QUAD=0: wavefront 0 alone)
    io.quad = (!rvo_form && e->cfg.max_agents <= kEvalQuadMaxAgents && k.tile_rows >= k.wpw * e->cfg.max_agents &&
               quad_lds_bytes<kEvalQuadMaxAgents>((k.tile_rows * k.width + 3) & ~3) <= (size_t)2 * kSpPlaneB) ? 1 : 0;
    if (const char *ov = std::getenv("CAVOID_ACTOR_QUAD")) io.quad = (io.quad && std::atoi(ov) != 0) ? 1 : 0;
    // every tile ADDS its running worlds on leaving: the word starts from zero, on the stream
    HIP_TRY(hipMemsetAsync(b->worlds_running, 0, sizeof(int32_t), s));
    const int rc_launch = frozen ? cavoid_launch_eval_frozen(e, sa, fz, io, s)
                                 : (rvo_form ? cavoid_launch_eval_rvo(e, sa, io, s) : launch_eval_any<false>(e, sa, sa, io, s));
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_eval_finish(h->step_counter, n_steps, s);
}

// eval_finish_kernel for the evaluation launches of other translation units too (cavoid_eval_ws.hip)
int cavoid_launch_eval_finish(int32_t *policy_step, int32_t n_steps, hipStream_t s) {
    hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(1), 0, s, policy_step, n_steps);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}
