// cavoid_crowd.hip -- the crowd step form (cavoid_crowd.hpp): every stepping, reset and observe launch of an env of more than
// kTileMaxAgents agents per world.  Two buckets of the agent count (17..32, 33..64) x four modes; N itself is a kernel argument.
// Own translation unit, compiled with -mllvm -disable-machine-licm like the other step loops (build.py).
#include "cavoid_launch.hpp"
#include "cavoid_crowd.hpp"

using namespace cavoid;

template <int NB, int MODE>
static void launch_crowd_mode(const cavoid_env *e, const KCfg &k, const KState &st, unsigned grid, size_t lds, const KIO &io, hipStream_t s,
                              hipEvent_t ev_start, hipEvent_t ev_stop) {
    launch_kernel(crowd_kernel<NB, MODE>, dim3(grid), dim3(64), lds, s, ev_start, ev_stop, k, st, (const PoolRec *)e->pool, io,
                  (int)e->cfg.max_agents);
}

template <int NB>
static int launch_crowd_nb(const cavoid_env *e, int mode, const KCfg &k, const KState &st, unsigned grid, size_t lds, const KIO &io, hipStream_t s,
                           hipEvent_t ev_start, hipEvent_t ev_stop) {
    switch (mode) {
        case MODE_STEP: launch_crowd_mode<NB, MODE_STEP>(e, k, st, grid, lds, io, s, ev_start, ev_stop); break;
        case MODE_STEP_AUTORESET:                                // one step or many: the same loop (restarts gathered on demand)
        case MODE_STEP_AUTORESET_PF:
        case MODE_STEP_AUTORESET_N: launch_crowd_mode<NB, MODE_STEP_AUTORESET_N>(e, k, st, grid, lds, io, s, ev_start, ev_stop); break;
        case MODE_OBSERVE: launch_crowd_mode<NB, MODE_OBSERVE>(e, k, st, grid, lds, io, s, ev_start, ev_stop); break;
        case MODE_RESET: launch_crowd_mode<NB, MODE_RESET>(e, k, st, grid, lds, io, s, ev_start, ev_stop); break;
        default: return CAVOID_EINVAL;
    }
    return CAVOID_OK;
}

int cavoid_launch_crowd(cavoid_env *e, int mode, const KCfg &k, const KState &st, int64_t worlds, const KIO &io, hipStream_t s,
                        hipEvent_t ev_start, hipEvent_t ev_stop) {
    const int n = e->cfg.max_agents;
    // ORCA agents may exist: the stepping launches take the kernels that carry the wave-cooperative solve (cavoid_crowd_rvo.hip)
    if (k.rvo_enabled && mode != MODE_OBSERVE && mode != MODE_RESET) return cavoid_launch_crowd_rvo(e, mode, k, st, worlds, io, s, ev_start, ev_stop);
    if (n < 2 || n > CAVOID_MAX_AGENTS || k.ahead > 0) return CAVOID_EUNSUPPORTED;
    const int64_t waves = (worlds + k.wpw - 1) / k.wpw;
    if (waves < 1 || waves > 0x7fffffffLL) return CAVOID_EINVAL;
    const int ostride = io.obs ? io.obs_stride : k.width;
    const size_t lds = (size_t)(lds_floats_block() + crowd_wave_floats(n, k.tile_rows, ostride)) * sizeof(float);
    if (lds > 65536) return CAVOID_EUNSUPPORTED;
    const int rc = n <= 32 ? launch_crowd_nb<32>(e, mode, k, st, (unsigned)waves, lds, io, s, ev_start, ev_stop)
                           : launch_crowd_nb<64>(e, mode, k, st, (unsigned)waves, lds, io, s, ev_start, ev_stop);
    if (rc != CAVOID_OK) return rc;
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}
