// cavoid_actor_host.hpp -- launch of actor_kernel<N, RVO, FROZEN> (cavoid_actor.hpp), shared by the two translation units that instantiate
// it: cavoid_actor.hip (RVO = false) and cavoid_actor_rvo.hip (RVO = true: ORCA agents, box scenarios generated inside the step).
#pragma once
#include <hip/hip_runtime.h>

#include "cavoid.h"
#include "cavoid_actor.hpp"
#include "cavoid_host.hpp"
#include "cavoid_launch.hpp"
#include "cavoid_loop_host.hpp"

namespace cavoid {

template <int N, bool RVO, bool FROZEN = false>
static int launch_actor(cavoid_env *e, const SplitArgs &sa, const SplitArgs &fz, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio, const ActorIO &io,
                        hipStream_t s) {
    return launch_big_lds<actor_kernel<N, RVO, FROZEN>>(e->device, policy_split_lds_bytes(), loop_tile_count(e), s, loop_kcfg(e, /*stream_obs=*/false), e->st,
                                                        e->pool, sa, fz, rc, rs, rio, io);
}

template <bool RVO, bool FROZEN = false>
static int launch_actor_any(cavoid_env *e, const SplitArgs &sa, const SplitArgs &fz, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio, const ActorIO &io,
                            hipStream_t s) {
    return dispatch_n(e->cfg.max_agents, EnvNs{}, [&](auto n) { return launch_actor<decltype(n)::value, RVO, FROZEN>(e, sa, fz, rc, rs, rio, io, s); });
}

template <int N, bool RVO>
static int launch_step_push(cavoid_env *e, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio, const ActorIO &io, int32_t step, hipStream_t s) {
    const KCfg &k = e->k;
    const size_t lds = (size_t)(lds_floats_block() + e->waves_per_block * (lds_floats_fixed(e->cfg.max_agents) + k.rvo_lds_floats + loop_tile_floats(k))) * sizeof(float);
    hipLaunchKernelGGL((step_push_kernel<N, RVO>), dim3((unsigned)e->grid, 2u), dim3(64 * e->waves_per_block), lds, s, k, e->st, e->pool, rc, rs, rio, io, step);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

template <bool RVO>
static int launch_step_push_any(cavoid_env *e, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio, const ActorIO &io, int32_t step,
                                hipStream_t s) {
    return dispatch_n(e->cfg.max_agents, EnvNs{}, [&](auto n) { return launch_step_push<decltype(n)::value, RVO>(e, rc, rs, rio, io, step, s); });
}

}  // namespace cavoid

// cavoid_actor_rvo.hip
int cavoid_launch_step_push_rvo(cavoid_env *e, const cavoid::RolloutCfg &rc, const cavoid::RolloutState &rs, const cavoid::RolloutIO &rio,
                                const cavoid::ActorIO &io, int32_t step, hipStream_t s);
int cavoid_launch_actor_rvo(cavoid_env *e, const cavoid::SplitArgs &sa, const cavoid::RolloutCfg &rc, const cavoid::RolloutState &rs,
                            const cavoid::RolloutIO &rio, const cavoid::ActorIO &io, hipStream_t s);
// cavoid_actor_frozen.hip: actor_kernel<N, true, true> -- the 'everything' instantiation (ORCA agents, in-step box scenarios) + a
// second, frozen network for the policy-4 agents
int cavoid_launch_actor_frozen(cavoid_env *e, const cavoid::SplitArgs &sa, const cavoid::SplitArgs &fz, const cavoid::RolloutCfg &rc,
                               const cavoid::RolloutState &rs, const cavoid::RolloutIO &rio, const cavoid::ActorIO &io, hipStream_t s);
// cavoid_crowd_push.hip: crowd_push_kernel<NB> -- cavoid_step_push on an env of more than kTileMaxAgents agents per world (the crowd step form);
// CAVOID_EUNSUPPORTED for a configuration the crowd form does not carry or whose LDS does not fit 64 KiB
int cavoid_launch_crowd_rvo_push(cavoid_env *e, const cavoid::RolloutCfg &rc, const cavoid::RolloutState &rs, const cavoid::RolloutIO &rio,
                                 const cavoid::ActorIO &io, int32_t step, hipStream_t s);   // (cavoid_crowd_rvo.hip: an env with rvo_enabled; cavoid_launch_crowd_push routes there)
int cavoid_launch_crowd_push(cavoid_env *e, const cavoid::RolloutCfg &rc, const cavoid::RolloutState &rs, const cavoid::RolloutIO &rio,
                             const cavoid::ActorIO &io, int32_t step, hipStream_t s);
// cavoid_crowd_actor.hip: crowd_actor_kernel<NB, RVO> -- cavoid_crowd_actor_run's launch (the closed loop of crowd worlds; routes an env with
// rvo_enabled to the ORCA-carrying instantiation); CAVOID_EUNSUPPORTED as cavoid_launch_crowd_push
int cavoid_launch_crowd_actor(cavoid_env *e, const cavoid::SplitArgs &sa, const cavoid::RolloutCfg &rc, const cavoid::RolloutState &rs,
                              const cavoid::RolloutIO &rio, const cavoid::ActorIO &io, hipStream_t s);
// cavoid_actor.hip: actor_finish_kernel behind an actor launch (the two device-side counters move on by n_steps; policy_step may be null)
int cavoid_launch_actor_finish(int32_t *rollout_step, int32_t *policy_step, int32_t n_steps, hipStream_t s);
