// cavoid_actor_ws_host.hpp -- launch of actor_ws_kernel<N, RVO> (cavoid_actor_ws.hpp), shared by the two translation units that
// instantiate it: cavoid_actor_ws.hip (RVO = false) and cavoid_actor_ws_rvo.hip (RVO = true: ORCA agents, box scenarios generated
// inside the step).
#pragma once
#include <hip/hip_runtime.h>

#include "cavoid.h"
#include "cavoid_actor_ws.hpp"
#include "cavoid_host.hpp"
#include "cavoid_launch.hpp"
#include "cavoid_loop_host.hpp"

namespace cavoid {

template <int N, bool RVO>
static int launch_actor_ws(cavoid_env *e, const PolicyWsArgs &wa, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio, const ActorIO &io,
                           hipStream_t s) {
    return launch_big_lds<actor_ws_kernel<N, RVO>>(e->device, policy_lds_bytes(4), loop_tile_count(e), s, loop_kcfg(e, /*stream_obs=*/false), e->st, e->pool, wa,
                                                   rc, rs, rio, io);
}

template <bool RVO>
static int launch_actor_ws_any(cavoid_env *e, const PolicyWsArgs &wa, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio, const ActorIO &io,
                               hipStream_t s) {
    return dispatch_n(e->cfg.max_agents, EnvNs{}, [&](auto n) { return launch_actor_ws<decltype(n)::value, RVO>(e, wa, rc, rs, rio, io, s); });
}

}  // namespace cavoid

// cavoid_actor_ws_rvo.hip
int cavoid_launch_actor_ws_rvo(cavoid_env *e, const cavoid::PolicyWsArgs &wa, const cavoid::RolloutCfg &rc, const cavoid::RolloutState &rs,
                               const cavoid::RolloutIO &rio, const cavoid::ActorIO &io, hipStream_t s);
