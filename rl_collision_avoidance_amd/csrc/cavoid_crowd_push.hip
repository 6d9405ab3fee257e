// cavoid_crowd_push.hip -- launch of crowd_push_kernel<NB> (cavoid_crowd_push.hpp): cavoid_step_push on an env of more than
// kTileMaxAgents agents per world.  Two buckets of the agent count (17..32, 33..64); N itself is a kernel argument.  Own translation
// unit, compiled with -mllvm -disable-machine-licm like cavoid_crowd.hip (build.py): the env step inside is the crowd form's step loop.
#include "cavoid_actor_host.hpp"
#include "cavoid_crowd_push.hpp"

using namespace cavoid;

int cavoid_launch_crowd_push(cavoid_env *e, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio, const ActorIO &io, int32_t step,
                             hipStream_t s) {
    const KCfg &k = e->k;
    const int n = e->cfg.max_agents;
    if (k.rvo_enabled) return cavoid_launch_crowd_rvo_push(e, rc, rs, rio, io, step, s);                // (cavoid_crowd_rvo.hip)
    if (n < 2 || n > CAVOID_MAX_AGENTS || k.ahead > 0) return CAVOID_EUNSUPPORTED;                      // (cavoid_launch_crowd's refusals)
    const int64_t tiles = (e->W + k.wpw - 1) / k.wpw;
    if (tiles < 1 || tiles > 0x7fffffffLL) return CAVOID_EINVAL;
    // one LDS allocation per workgroup, crowd_kernel's: only the env wavefront uses it
    const size_t lds = (size_t)(lds_floats_block() + crowd_wave_floats(n, k.tile_rows, k.width)) * sizeof(float);
    if (lds > 65536) return CAVOID_EUNSUPPORTED;
    if (n <= 32)
        hipLaunchKernelGGL(crowd_push_kernel<32>, dim3((unsigned)tiles), dim3(128), lds, s, k, e->st, (const PoolRec *)e->pool, rc, rs, rio, io, n, step);
    else
        hipLaunchKernelGGL(crowd_push_kernel<64>, dim3((unsigned)tiles), dim3(128), lds, s, k, e->st, (const PoolRec *)e->pool, rc, rs, rio, io, n, step);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}
