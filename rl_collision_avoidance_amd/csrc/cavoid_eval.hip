// cavoid_eval.hip -- C ABI (include/cavoid.h, cavoid_eval_run) over eval_kernel<N> (cavoid_eval.hpp): K evaluation steps -- policy forward,
// action selection, env.step without auto-reset, outcome record -- in ONE launch that finished tiles leave early.  Own translation unit (the
// kernel carries the policy's GEMM loops and the env step; instantiated per agent count).
#define CAVOID_EVAL_KERNELS
#include "cavoid_eval_host.hpp"
#include "cavoid_policy_host.hpp"

using namespace cavoid;

extern "C" int cavoid_eval_run(cavoid_env *e, cavoid_policy *h, cavoid_policy *frozen, const cavoid_eval_buffers *b, float *obs, float *rewards,
                               uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps, int32_t greedy, void *stream) {
    if (!eval_args_ok(e, h, b, obs, rewards, done, game_over, actions, values, n_steps)) return CAVOID_EINVAL;
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
    const bool rvo_form = loop_rvo_form(e);                   // actor_run's routing
    // the env step borrows the (idle) activation planes: staging arrays + obs tile (+ the ORCA lines)
    const size_t lent = (size_t)2 * kSpPlaneB;
    if (eval_env_lds_bytes(e->cfg.max_agents, loop_tile_floats(e->k), e->k.rvo_lds_floats) > lent) return CAVOID_EUNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);

    const SplitArgs sa = split_args(e, h);
    EvalIO io = eval_io(b, obs, rewards, done, game_over, actions, values, n_steps, greedy);
    io.quad = quad_form<kEvalQuadMaxAgents>(e, rvo_form, lent);      // (where actor_run takes that form)
    // every tile ADDS its running worlds on leaving: the word starts from zero, on the stream
    HIP_TRY(hipMemsetAsync(b->worlds_running, 0, sizeof(int32_t), s));
    const int rc_launch = frozen ? cavoid_launch_eval_frozen(e, sa, frozen_split_args(sa, frozen), io, s)
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
