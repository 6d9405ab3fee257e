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

namespace cavoid {

template <int N, bool RVO, bool FROZEN = false>
static int launch_eval_ws(cavoid_env *e, const PolicyWsArgs &wa, const PolicyWsArgs &fz, const EvalIO &io, hipStream_t s) {
    // > 64 KiB of dynamic LDS: opted into once per instantiation AND device (as launch_eval, cavoid_eval_host.hpp)
    static bool opted_in[64] = {};
    const int dev = e->device;
    if (dev < 0 || dev >= 64 || !opted_in[dev]) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(eval_ws_kernel<N, RVO, FROZEN>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)eval_ws_lds_bytes()));
        if (dev >= 0 && dev < 64) opted_in[dev] = true;
    }
    const int64_t tiles = (e->W + e->k.wpw - 1) / e->k.wpw;
    KCfg k = e->k;
    k.stream_obs = 0;                                        // (the tile's own policy phase reads the rows next: they stay in the L2)
    hipLaunchKernelGGL((eval_ws_kernel<N, RVO, FROZEN>), dim3((unsigned)tiles), dim3(256), eval_ws_lds_bytes(), s, k, e->st, e->pool, wa, fz, io);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
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
