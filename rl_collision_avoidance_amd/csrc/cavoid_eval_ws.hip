// cavoid_eval_ws.hip -- C ABI (include/cavoid.h, cavoid_eval_run_ws) over eval_ws_kernel<N> (cavoid_eval_ws.hpp): K evaluation steps of the
// weight-sharing network -- policy forward, action selection, env.step without auto-reset, outcome record -- in ONE launch that finished
// tiles leave early.  Own translation unit (the kernel carries the weight-sharing pass and the env step; instantiated per agent count).
#include "cavoid_eval_ws_host.hpp"
#include "cavoid_policy_host.hpp"

using namespace cavoid;

// a handle the kernel's pass runs on: the weight-sharing network on the whole parked row (an LSTM handle has cavoid_eval_run, a ring
// handle -- cavoid_policy_create_ws_crowd, 20..64 neighbours -- evaluates step by step)
static bool whole_row_ws(const cavoid_policy *h) { return h->ws && !h->crowd && h->max_other <= kWsMaxOthers; }

extern "C" int cavoid_eval_run_ws(cavoid_env *e, cavoid_policy *h, cavoid_policy *frozen, const cavoid_eval_buffers *b, float *obs, float *rewards,
                                  uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps, int32_t greedy, void *stream) {
    if (!eval_args_ok(e, h, b, obs, rewards, done, game_over, actions, values, n_steps)) return CAVOID_EINVAL;
    if (!whole_row_ws(h) || (frozen && !whole_row_ws(frozen))) return CAVOID_EUNSUPPORTED;
    if (n_steps == 0) return CAVOID_OK;
    if (!h->loaded) return CAVOID_EINVAL;
    // the handles must describe the same batch
    if (h->device != e->device || h->in_size != e->k.width - 1 || h->max_other != e->cfg.max_other) return CAVOID_EINVAL;
    // what the kernel does not carry -- exactly what cavoid_actor_run_ws refuses (cavoid_actor_ws.hip): crowd worlds, velocity actions
    if (e->cfg.max_agents > kTileMaxAgents) return CAVOID_EUNSUPPORTED;
    if (e->cfg.dynamics == CAVOID_DYN_HOLONOMIC) return CAVOID_EUNSUPPORTED;
    // frozen-network agents act by THEIR network: without it this entry point would hand them action 0
    if (!frozen && e->cfg.gen_frozen_fraction > 0.0 && e->cfg.gen_nonlearning_fraction > 0.0) return CAVOID_EUNSUPPORTED;
    if (frozen && (!frozen->loaded || frozen->device != e->device || frozen->in_size != h->in_size || frozen->max_other != h->max_other ||
                   frozen->num_actions != h->num_actions))
        return frozen->loaded ? CAVOID_EUNSUPPORTED : CAVOID_EINVAL;
    const bool rvo_form = loop_rvo_form(e);                   // actor_run_ws's routing
    // the env step borrows the (idle) activation rows: staging arrays + obs tile (+ the ORCA lines)
    const size_t lent = actor_ws_lent_bytes();
    if (eval_env_lds_bytes(e->cfg.max_agents, loop_tile_floats(e->k), e->k.rvo_lds_floats) > lent) return CAVOID_EUNSUPPORTED;
    HIP_TRY(hipSetDevice(e->device));
    // (no cavoid_ahead_prepare: nothing restarts)
    hipStream_t s = static_cast<hipStream_t>(stream);

    PolicyWsArgs wa{};
    wa.a = loop_policy_args(e, h);
    PolicyWsArgs fz = wa;                                    // the frozen network: same shapes, its own weights / normalisation; argmax only
    if (frozen) fz.a = frozen_ws_args(e, frozen);
    EvalIO io = eval_io(b, obs, rewards, done, game_over, actions, values, n_steps, greedy);
    io.quad = quad_form<kEvalQuadMaxAgents>(e, rvo_form, lent);      // (where cavoid_actor_run_ws takes that form, inside the lent rows)
    // every tile ADDS its running worlds on leaving: the word starts from zero, on the stream
    HIP_TRY(hipMemsetAsync(b->worlds_running, 0, sizeof(int32_t), s));
    const int rc_launch = frozen ? cavoid_launch_eval_ws_frozen(e, wa, fz, io, s)
                                 : (rvo_form ? cavoid_launch_eval_ws_rvo(e, wa, io, s) : launch_eval_ws_any<false>(e, wa, wa, io, s));
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_eval_finish(h->step_counter, n_steps, s);
}
