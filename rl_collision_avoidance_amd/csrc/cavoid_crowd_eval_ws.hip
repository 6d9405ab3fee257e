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

template <int NB, bool RVO, bool FROZEN>
static int launch_crowd_ws_eval(cavoid_env *e, unsigned tiles, const PolicyWsArgs &wa, const PolicyWsArgs &fz, const EvalIO &io, hipStream_t s) {
    // > 64 KiB of dynamic LDS: opted into once per instantiation and device (see launch_actor)
    static bool opted_in[64] = {};
    const int dev = e->device;
    if (dev < 0 || dev >= 64 || !opted_in[dev]) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(crowd_ws_evaluate_kernel<NB, RVO, FROZEN>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)eval_ws_lds_bytes()));
        if (dev >= 0 && dev < 64) opted_in[dev] = true;
    }
    KCfg k = e->k;
    k.stream_obs = 0;                                        // (the tile's own policy phase reads the rows next: they stay in the L2)
    hipLaunchKernelGGL((crowd_ws_evaluate_kernel<NB, RVO, FROZEN>), dim3(tiles), dim3(256), eval_ws_lds_bytes(), s, k, e->st, (const PoolRec *)e->pool,
                       wa, fz, io, e->cfg.max_agents);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

template <bool FROZEN>
static int launch_crowd_ws_eval_any(cavoid_env *e, const PolicyWsArgs &wa, const PolicyWsArgs &fz, const EvalIO &io, hipStream_t s) {
    const KCfg &k = e->k;
    const int n = e->cfg.max_agents;
    if (!crowd_form(n) || n < 2 || n > CAVOID_MAX_AGENTS) return CAVOID_EUNSUPPORTED;
    const int64_t tiles = (e->W + k.wpw - 1) / k.wpw;
    if (tiles < 1 || tiles > 0x7fffffffLL) return CAVOID_EINVAL;
    // the env step borrows the (idle) activation rows: crowd_kernel's allocation, at most 64 KB of the rows' 65 KB -- the row list and
    // EvalShared behind them survive it
    const size_t lds = crowd_actor_env_lds_bytes(n, k.tile_rows, k.width);
    if (lds > 65536 || lds > actor_ws_lent_bytes()) return CAVOID_EUNSUPPORTED;
    // every tile ADDS its running worlds on leaving: the word starts from zero, on the stream
    HIP_TRY(hipMemsetAsync(io.worlds_running, 0, sizeof(int32_t), s));
    // an env whose worlds may hold ORCA agents (cfg.rvo_enabled = CAVOID_RVO_WAVE): the ORCA-carrying env step, as cavoid_launch_crowd routes
    if (k.rvo_enabled)
        return n <= 32 ? launch_crowd_ws_eval<32, true, FROZEN>(e, (unsigned)tiles, wa, fz, io, s)
                       : launch_crowd_ws_eval<64, true, FROZEN>(e, (unsigned)tiles, wa, fz, io, s);
    return n <= 32 ? launch_crowd_ws_eval<32, false, FROZEN>(e, (unsigned)tiles, wa, fz, io, s)
                   : launch_crowd_ws_eval<64, false, FROZEN>(e, (unsigned)tiles, wa, fz, io, s);
}

extern "C" int cavoid_crowd_eval_run_ws(cavoid_env *e, cavoid_policy *h, cavoid_policy *frozen, const cavoid_eval_buffers *b, float *obs, float *rewards,
                                        uint8_t *done, uint8_t *game_over, int32_t *actions, float *values, int32_t n_steps, int32_t greedy,
                                        void *stream) {
    if (!e || !h || !b || b->struct_size != (int32_t)sizeof(cavoid_eval_buffers) || !obs || !rewards || !done || !game_over || !actions || !values ||
        n_steps < 0)
        return CAVOID_EINVAL;
    if (!b->ret || !b->goal_step || !b->world_steps || !b->worlds_running) return CAVOID_EINVAL;
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
    wa.a = policy_common_args(h, nullptr, e->A, e->k.width);   // (x: the observation buffer, set by the kernel)
    wa.a.seed_lo = (uint32_t)h->seed; wa.a.seed_hi = (uint32_t)(h->seed >> 32);
    wa.a.step_counter = h->step_counter; wa.a.blocks_done = h->blocks_done;
    PolicyWsArgs fz = wa;                                    // the frozen network: same shapes, its own weights / normalisation; argmax only
    if (frozen) fz.a = policy_common_args(frozen, nullptr, e->A, e->k.width);
    EvalIO io{};
    io.obs = obs; io.rewards = rewards; io.done = done; io.game_over = game_over; io.actions = actions; io.values = values;
    io.ret = b->ret; io.goal_step = b->goal_step; io.world_steps = b->world_steps; io.worlds_running = b->worlds_running;
    io.n_steps = n_steps; io.greedy = greedy ? 1 : 0;
    e->last_form = CAVOID_FORM_NONE;
    const int rc_raw = frozen ? launch_crowd_ws_eval_any<true>(e, wa, fz, io, s) : launch_crowd_ws_eval_any<false>(e, wa, wa, io, s);
    const int rc_launch = note_form(e, rc_raw, crowd_step_form(e));     // (reported as after cavoid_step)
    if (rc_launch != CAVOID_OK) return rc_launch;
    return cavoid_launch_eval_finish(h->step_counter, n_steps, s);
}
