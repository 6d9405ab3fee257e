// cavoid_eval_host.hpp -- launch of eval_kernel<N, RVO, FROZEN> (cavoid_eval.hpp), shared by the three translation units that instantiate
// it: cavoid_eval.hip (the plain env step), cavoid_eval_rvo.hip (ORCA agents) and cavoid_eval_frozen.hip (ORCA + frozen-network agents).
#pragma once
#include <hip/hip_runtime.h>

#include "cavoid.h"
#include "cavoid_eval.hpp"
#include "cavoid_host.hpp"
#include "cavoid_launch.hpp"
#include "cavoid_loop_host.hpp"

namespace cavoid {

template <int N, bool RVO, bool FROZEN = false>
static int launch_eval(cavoid_env *e, const SplitArgs &sa, const SplitArgs &fz, const EvalIO &io, hipStream_t s) {
    return launch_big_lds<eval_kernel<N, RVO, FROZEN>>(e->device, eval_lds_bytes(), loop_tile_count(e), s, loop_kcfg(e, /*stream_obs=*/false), e->st, e->pool, sa,
                                                       fz, io);
}

template <bool RVO, bool FROZEN = false>
static int launch_eval_any(cavoid_env *e, const SplitArgs &sa, const SplitArgs &fz, const EvalIO &io, hipStream_t s) {
    return dispatch_n(e->cfg.max_agents, EnvNs{}, [&](auto n) { return launch_eval<decltype(n)::value, RVO, FROZEN>(e, sa, fz, io, s); });
}

}  // namespace cavoid

// cavoid_eval_rvo.hip: eval_kernel<N, true>
int cavoid_launch_eval_rvo(cavoid_env *e, const cavoid::SplitArgs &sa, const cavoid::EvalIO &io, hipStream_t s);
// cavoid_eval_frozen.hip: eval_kernel<N, true, true> -- the 'everything' env step + a second, frozen network for the policy-4 agents
int cavoid_launch_eval_frozen(cavoid_env *e, const cavoid::SplitArgs &sa, const cavoid::SplitArgs &fz, const cavoid::EvalIO &io, hipStream_t s);
// cavoid_eval.hip: eval_finish_kernel behind an evaluation launch, for both entry points (cavoid_eval_run, cavoid_eval_run_ws)
int cavoid_launch_eval_finish(int32_t *policy_step, int32_t n_steps, hipStream_t s);
