// cavoid_crowd_eval.hip -- C ABI (include/cavoid.h, cavoid_crowd_eval_run) over crowd_evaluate_kernel<NB, RVO> (cavoid_crowd_eval.hpp): cavoid_eval_run
// for an env of more than kTileMaxAgents agents per world.  Two buckets of the agent count (17..32, 33..64) x (plain, ORCA-carrying env step);
// N itself is a kernel argument.  Own translation unit, compiled with -mllvm -disable-machine-licm like every other step-loop unit
// (build.py): the kernel runs policy + env step + outcome record inside one step loop.
#include "cavoid_crowd_eval.hpp"
#include "cavoid_eval_host.hpp"
#include "cavoid_policy_host.hpp"

using namespace cavoid;

static int launch_crowd_eval_any(cavoid_env *e, const SplitArgs &sa, const EvalIO &io, hipStream_t s) {
    // the env step borrows the (idle) activation planes: crowd_kernel's allocation, what cavoid_launch_crowd_actor allows
    unsigned tiles = 0;
    if (int rc_t = crowd_loop_tiles(e, /*lent=*/(size_t)2 * kSpPlaneB, /*refuse_ahead=*/false, &tiles)) return rc_t;
    // every tile ADDS its running worlds on leaving: the word starts from zero, on the stream
    HIP_TRY(hipMemsetAsync(io.worlds_running, 0, sizeof(int32_t), s));
    return dispatch_crowd_bucket(e->cfg.max_agents, e->k.rvo_enabled != 0, [&](auto nb, auto rvo) {
        return launch_big_lds<crowd_evaluate_kernel<decltype(nb)::value, decltype(rvo)::value>>(
            e->device, eval_lds_bytes(), tiles, s, loop_kcfg(e, /*stream_obs=*/false), e->st, (const PoolRec *)e->pool, sa, io, e->cfg.max_agents);
    });
}

extern "C" int cavoid_crowd_eval_run(cavoid_env *e, cavoid_policy *h, const cavoid_eval_buffers *b, float *obs, float *rewards, uint8_t *done,
                                     uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps, int32_t greedy, void *stream) {
    if (!eval_args_ok(e, h, b, obs, rewards, done, game_over, actions, values, n_steps)) return CAVOID_EINVAL;
    if (h->ws) return CAVOID_EUNSUPPORTED;                   // (the kernel embeds the LSTM pass: a weight-sharing handle evaluates step by step)
    if (n_steps == 0) return CAVOID_OK;
    if (!h->loaded) return CAVOID_EINVAL;
    // the handles must describe the same batch
    if (h->device != e->device || h->in_size != e->k.width - 1 || h->max_other != e->cfg.max_other) return CAVOID_EINVAL;
    // what the kernel does not carry -- exactly what cavoid_crowd_actor_run refuses (cavoid_actor.hip), for the same reasons; tile worlds
    // have cavoid_eval_run
    if (e->cfg.dynamics == CAVOID_DYN_HOLONOMIC || !h->use_split || h->split_products != kSpDefaultProducts) return CAVOID_EUNSUPPORTED;
    if (e->cfg.max_agents <= kTileMaxAgents) return CAVOID_EUNSUPPORTED;
    // frozen-network agents act by THEIR network, and this launch carries one (there is no frozen form of it)
    if (e->cfg.gen_frozen_fraction > 0.0 && e->cfg.gen_nonlearning_fraction > 0.0) return CAVOID_EUNSUPPORTED;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (no cavoid_ahead_prepare: nothing restarts)

    const SplitArgs sa = split_args(e, h);
    const EvalIO io = eval_io(b, obs, rewards, done, game_over, actions, values, n_steps, greedy);
    e->last_form = CAVOID_FORM_NONE;
    const int rc_launch = note_form(e, launch_crowd_eval_any(e, sa, io, s), crowd_step_form(e));     // (reported as after cavoid_step)
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_eval_finish(h->step_counter, n_steps, s);
}
