// cavoid_actor_ws_host.hpp -- launch of actor_ws_kernel<N, RVO> (cavoid_actor_ws.hpp), shared by the two translation units that
// instantiate it: cavoid_actor_ws.hip (RVO = false) and cavoid_actor_ws_rvo.hip (RVO = true: ORCA agents, box scenarios generated
// inside the step).
#pragma once
#include <hip/hip_runtime.h>

#include "cavoid.h"
#include "cavoid_actor_ws.hpp"
#include "cavoid_host.hpp"
#include "cavoid_launch.hpp"

namespace cavoid {

template <int N, bool RVO>
static int launch_actor_ws(cavoid_env *e, const PolicyWsArgs &wa, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio, const ActorIO &io,
                           hipStream_t s) {
    // > 64 KiB of dynamic LDS: opted into once per instantiation AND device (as launch_actor, cavoid_actor_host.hpp)
    static bool opted_in[64] = {};
    const int dev = e->device;
    if (dev < 0 || dev >= 64 || !opted_in[dev]) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(actor_ws_kernel<N, RVO>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)policy_lds_bytes(4)));
        if (dev >= 0 && dev < 64) opted_in[dev] = true;
    }
    const int64_t tiles = (e->W + e->k.wpw - 1) / e->k.wpw;
    KCfg k = e->k;
    k.stream_obs = 0;                                        // (the tile's own policy phase reads the rows next: they stay in the L2)
    hipLaunchKernelGGL((actor_ws_kernel<N, RVO>), dim3((unsigned)tiles), dim3(256), policy_lds_bytes(4), s, k, e->st, e->pool, wa, rc, rs, rio, io);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
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
