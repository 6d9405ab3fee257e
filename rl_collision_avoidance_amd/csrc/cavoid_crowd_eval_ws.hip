// cavoid_crowd_eval_ws.hip -- C ABI (include/cavoid.h, cavoid_crowd_eval_run_ws) over crowd_ws_evaluate_kernel<NB, RVO, FROZEN>
// (cavoid_crowd_eval_ws.hpp): cavoid_eval_run_ws for an env of more than kTileMaxAgents agents per world -- K evaluation steps of crowd worlds
// with the weight-sharing network (the ring form of the pass on the tile's live rows, action selection, the crowd env step without
// auto-reset, the outcome record) in ONE launch that finished tiles leave early.  Two buckets of the agent count (17..32, 33..64) x
// (plain, ORCA-carrying env step) x (one network, a second frozen one); N itself is a kernel argument, and the one ring instantiation of
// the pass serves every neighbour count 1..64.  Own translation unit, compiled with -mllvm -disable-machine-licm like every other
// step-loop unit (build.py).
#include "cavoid_crowd_eval_ws.hpp"
#include "cavoid_eval_host.hpp"
#include "cavoid_policy_host.hpp"

using namespace cavoid;

template <bool FROZEN>
static int launch_crowd_ws_eval_any(cavoid_env *e, const PolicyWsArgs &wa, const PolicyWsArgs &fz, const EvalIO &io, hipStream_t s) {
    // the env step borrows the (idle) activation rows: crowd_kernel's allocation, at most 64 KB of the rows' 65 KB -- the row list and
    // EvalShared behind them survive it
    unsigned tiles = 0;
    if (int rc_t = crowd_loop_tiles(e, /*lent=*/actor_ws_lent_bytes(), /*refuse_ahead=*/false, &tiles)) return rc_t;
    // every tile ADDS its running worlds on leaving: the word starts from zero, on the stream
    HIP_TRY(hipMemsetAsync(io.worlds_running, 0, sizeof(int32_t), s));
    return dispatch_crowd_bucket(e->cfg.max_agents, e->k.rvo_enabled != 0, [&](auto nb, auto rvo) {
        return launch_big_lds<crowd_ws_evaluate_kernel<decltype(nb)::value, decltype(rvo)::value, FROZEN>>(
            e->device, eval_ws_lds_bytes(), tiles, s, loop_kcfg(e, /*stream_obs=*/false), e->st, (const PoolRec *)e->pool, wa, fz, io, e->cfg.max_agents);
    });
}

extern "C" int cavoid_crowd_eval_run_ws(cavoid_env *e, cavoid_policy *h, cavoid_policy *frozen, const cavoid_eval_buffers *b, float *obs, float *rewards,
                                        uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps, int32_t greedy,
                                        void *stream) {
    if (!eval_args_ok(e, h, b, obs, rewards, done, game_over, actions, values, n_steps)) return CAVOID_EINVAL;
    // the kernel embeds the weight-sharing pass in its ring form, which serves a cavoid_policy_create_ws handle (1..19 neighbours) and a
    // cavoid_policy_create_ws_crowd handle (20..64) alike: an LSTM handle has cavoid_crowd_eval_run
    if (!h->ws || h->max_other > kWsMaxOthersCrowd) return CAVOID_EUNSUPPORTED;
    if (n_steps == 0) return CAVOID_OK;
    if (!h->loaded) return CAVOID_EINVAL;
    // the handles must describe the same batch
    if (h->device != e->device || h->in_size != e->k.width - 1 || h->max_other != e->cfg.max_other) return CAVOID_EINVAL;
    // what the kernel does not carry: tile worlds (cavoid_eval_run_ws carries those), velocity actions
    if (e->cfg.max_agents <= kTileMaxAgents) return CAVOID_EUNSUPPORTED;
    if (e->cfg.dynamics == CAVOID_DYN_HOLONOMIC) return CAVOID_EUNSUPPORTED;
    // the frozen network: a weight-sharing handle (of either kind) of the learner's shape
    if (frozen) {
        if (!frozen->ws) return CAVOID_EUNSUPPORTED;
        if (!frozen->loaded) return CAVOID_EINVAL;
        if (frozen->device != e->device || frozen->in_size != h->in_size || frozen->max_other != h->max_other || frozen->num_actions != h->num_actions)
            return CAVOID_EUNSUPPORTED;
    }
    // frozen-network agents act by THEIR network: without it this entry point would hand them action 0
    if (!frozen && e->cfg.gen_frozen_fraction > 0.0 && e->cfg.gen_nonlearning_fraction > 0.0) return CAVOID_EUNSUPPORTED;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (no cavoid_ahead_prepare: nothing restarts)

    PolicyWsArgs wa{};
    wa.a = loop_policy_args(e, h);
    PolicyWsArgs fz = wa;                                    // the frozen network: same shapes, its own weights / normalisation; argmax only
    if (frozen) fz.a = frozen_ws_args(e, frozen);
    const EvalIO io = eval_io(b, obs, rewards, done, game_over, actions, values, n_steps, greedy);
    e->last_form = CAVOID_FORM_NONE;
    const int rc_raw = frozen ? launch_crowd_ws_eval_any<true>(e, wa, fz, io, s) : launch_crowd_ws_eval_any<false>(e, wa, wa, io, s);
    const int rc_launch = note_form(e, rc_raw, crowd_step_form(e));     // (reported as after cavoid_step)
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_eval_finish(h->step_counter, n_steps, s);
}
