// cavoid_crowd_actor.hip -- launch of crowd_actor_kernel<NB, RVO> (cavoid_crowd_actor.hpp): cavoid_crowd_actor_run (cavoid_actor.hip) on an env
// of more than kTileMaxAgents agents per world.  Two buckets of the agent count (17..32, 33..64) x (plain, ORCA-carrying env step); N itself
// is a kernel argument.  Own translation unit, compiled with -mllvm -disable-machine-licm like every other step-loop unit (build.py): the
// kernel runs policy + env step + bookkeeping inside one step loop.
#include "cavoid_actor_host.hpp"
#include "cavoid_crowd_actor.hpp"

using namespace cavoid;

template <int NB, bool RVO>
static int launch_crowd_actor(cavoid_env *e, unsigned tiles, const SplitArgs &sa, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio,
                              const ActorIO &io, hipStream_t s) {
    // > 64 KiB of dynamic LDS: opted into once per instantiation and device (see launch_actor)
    static bool opted_in[64] = {};
    const int dev = e->device;
    if (dev < 0 || dev >= 64 || !opted_in[dev]) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(crowd_actor_kernel<NB, RVO>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)policy_split_lds_bytes()));
        if (dev >= 0 && dev < 64) opted_in[dev] = true;
    }
    hipLaunchKernelGGL((crowd_actor_kernel<NB, RVO>), dim3(tiles), dim3(256), policy_split_lds_bytes(), s, e->k, e->st, (const PoolRec *)e->pool, sa, rc, rs,
                       rio, io, e->cfg.max_agents);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

int cavoid_launch_crowd_actor(cavoid_env *e, const SplitArgs &sa, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio, const ActorIO &io,
                              hipStream_t s) {
    const KCfg &k = e->k;
    const int n = e->cfg.max_agents;
    if (!crowd_form(n) || n < 2 || n > CAVOID_MAX_AGENTS || k.ahead > 0) return CAVOID_EUNSUPPORTED;    // (cavoid_launch_crowd_push's refusals)
    const int64_t tiles = (e->W + k.wpw - 1) / k.wpw;
    if (tiles < 1 || tiles > 0x7fffffffLL) return CAVOID_EINVAL;
    // the env step borrows the (idle) activation planes: crowd_kernel's allocation, at most 64 KB of the planes' 66 KB -- the live mask
    // behind the planes survives it
    const size_t lds = crowd_actor_env_lds_bytes(n, k.tile_rows, k.width);
    if (lds > 65536 || lds > (size_t)2 * kSpPlaneB) return CAVOID_EUNSUPPORTED;
    // an env whose worlds may hold ORCA agents (cfg.rvo_enabled = CAVOID_RVO_WAVE): the ORCA-carrying env step, as cavoid_launch_crowd_push routes
    if (k.rvo_enabled)
        return n <= 32 ? launch_crowd_actor<32, true>(e, (unsigned)tiles, sa, rc, rs, rio, io, s) : launch_crowd_actor<64, true>(e, (unsigned)tiles, sa, rc, rs, rio, io, s);
    return n <= 32 ? launch_crowd_actor<32, false>(e, (unsigned)tiles, sa, rc, rs, rio, io, s) : launch_crowd_actor<64, false>(e, (unsigned)tiles, sa, rc, rs, rio, io, s);
}
