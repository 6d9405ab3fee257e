// cavoid_eval_ws_host.hpp -- launch of eval_ws_kernel<N, RVO, FROZEN> (cavoid_eval_ws.hpp), shared by the three translation units that
// instantiate it: cavoid_eval_ws.hip (the plain env step), cavoid_eval_ws_rvo.hip (ORCA agents) and cavoid_eval_ws_frozen.hip (ORCA +
// frozen-network agents).
#pragma once
#include <hip/hip_runtime.h>

#include "cavoid.h"
#include "cavoid_eval_host.hpp"                              // (cavoid_launch_eval_finish)
#include "cavoid_eval_ws.hpp"
#include "cavoid_host.hpp"
#include "cavoid_launch.hpp"
#include "cavoid_loop_host.hpp"

namespace cavoid {

template <int N, bool RVO, bool FROZEN = false>
static int launch_eval_ws(cavoid_env *e, const PolicyWsArgs &wa, const PolicyWsArgs &fz, const EvalIO &io, hipStream_t s) {
    return launch_big_lds<eval_ws_kernel<N, RVO, FROZEN>>(e->device, eval_ws_lds_bytes(), loop_tile_count(e), s, loop_kcfg(e, /*stream_obs=*/false), e->st, e->pool,
                                                          wa, fz, io);
}

template <bool RVO, bool FROZEN = false>
static int launch_eval_ws_any(cavoid_env *e, const PolicyWsArgs &wa, const PolicyWsArgs &fz, const EvalIO &io, hipStream_t s) {
    return dispatch_n(e->cfg.max_agents, EnvNs{}, [&](auto n) { return launch_eval_ws<decltype(n)::value, RVO, FROZEN>(e, wa, fz, io, s); });
}

}  // namespace cavoid

// cavoid_eval_ws_rvo.hip: eval_ws_kernel<N, true>
int cavoid_launch_eval_ws_rvo(cavoid_env *e, const cavoid::PolicyWsArgs &wa, const cavoid::EvalIO &io, hipStream_t s);
// cavoid_eval_ws_frozen.hip: eval_ws_kernel<N, true, true> -- the 'everything' env step + a second, frozen network for the policy-4 agents
int cavoid_launch_eval_ws_frozen(cavoid_env *e, const cavoid::PolicyWsArgs &wa, const cavoid::PolicyWsArgs &fz, const cavoid::EvalIO &io, hipStream_t s);
