// cavoid_eval_host.hpp -- launch of eval_kernel<N, RVO, FROZEN> (cavoid_eval.hpp), shared by the three translation units that instantiate
// it: cavoid_eval.hip (the plain env step), cavoid_eval_rvo.hip (ORCA agents) and cavoid_eval_frozen.hip (ORCA + frozen-network agents).
#pragma once
#include <hip/hip_runtime.h>

#include "cavoid.h"
#include "cavoid_eval.hpp"
#include "cavoid_host.hpp"
#include "cavoid_launch.hpp"

namespace cavoid {

template <int N, bool RVO, bool FROZEN = false>
static int launch_eval(cavoid_env *e, const SplitArgs &sa, const SplitArgs &fz, const EvalIO &io, hipStream_t s) {
    // > 64 KiB of dynamic LDS: opted into once per instantiation AND device (launch_actor's note, cavoid_actor_host.hpp)
    static bool opted_in[64] = {};
    const int dev = e->device;
    if (dev < 0 || dev >= 64 || !opted_in[dev]) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(eval_kernel<N, RVO, FROZEN>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)eval_lds_bytes()));
        if (dev >= 0 && dev < 64) opted_in[dev] = true;
    }
    const int64_t tiles = (e->W + e->k.wpw - 1) / e->k.wpw;
    KCfg k = e->k;
    k.stream_obs = 0;                                        // (the tile's own policy phase reads the rows next: they stay in the L2)
    hipLaunchKernelGGL((eval_kernel<N, RVO, FROZEN>), dim3((unsigned)tiles), dim3(256), eval_lds_bytes(), s, k, e->st, e->pool, sa, fz, io);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
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
