// cavoid_crowd_rvo.hip -- the crowd step form's ORCA-carrying kernels (cavoid_crowd_rvo.hpp; CAVOID_FORM_CROWD_RVO): the stepping launches
// of an env of more than kTileMaxAgents agents per world with cfg.rvo_enabled = CAVOID_RVO_WAVE.  crowd_rvo_kernel: two buckets of the
// agent count (17..32, 33..64) x (MODE_STEP, MODE_STEP_AUTORESET_N); crowd_rvo_push_kernel: cavoid_step_push's one launch, two buckets.
// Reset and observe of such an env stay on crowd_kernel (cavoid_crowd.hip).  Own translation unit, compiled with
// -mllvm -disable-machine-licm like cavoid_crowd.hip (build.py): the same step loop.
#include "cavoid_actor_host.hpp"
#include "cavoid_crowd_push.hpp"

using namespace cavoid;

static size_t crowd_rvo_lds(int n, int tile_rows, int ostride) {
    static_assert(crowd_rvo_line_floats(2) <= crowd_key_floats(2) && crowd_rvo_line_floats(CAVOID_MAX_AGENTS) <= crowd_key_floats(CAVOID_MAX_AGENTS),
                  "one host's two line sets lie in the sort keys' region");
    return (size_t)(lds_floats_block() + crowd_wave_floats(n, tile_rows, ostride)) * sizeof(float);    // (crowd_kernel's: nothing added)
}

template <int NB>
static int launch_crowd_rvo_nb(const cavoid_env *e, int mode, const KCfg &k, const KState &st, unsigned grid, size_t lds, const KIO &io, hipStream_t s,
                               hipEvent_t ev_start, hipEvent_t ev_stop) {
    const PoolRec *pool = (const PoolRec *)e->pool;
    const int n = e->cfg.max_agents;
    switch (mode) {
        case MODE_STEP: launch_kernel(crowd_rvo_kernel<NB, MODE_STEP>, dim3(grid), dim3(64), lds, s, ev_start, ev_stop, k, st, pool, io, n); break;
        case MODE_STEP_AUTORESET:                                // one step or many: the same loop, as in cavoid_crowd.hip
        case MODE_STEP_AUTORESET_PF:
        case MODE_STEP_AUTORESET_N:
            launch_kernel(crowd_rvo_kernel<NB, MODE_STEP_AUTORESET_N>, dim3(grid), dim3(64), lds, s, ev_start, ev_stop, k, st, pool, io, n);
            break;
        default: return CAVOID_EINVAL;                           // (reset / observe: crowd_kernel)
    }
    return CAVOID_OK;
}

int cavoid_launch_crowd_rvo(cavoid_env *e, int mode, const KCfg &k, const KState &st, int64_t worlds, const KIO &io, hipStream_t s,
                            hipEvent_t ev_start, hipEvent_t ev_stop) {
    const int n = e->cfg.max_agents;
    if (!crowd_form(n) || n < 2 || n > CAVOID_MAX_AGENTS || !k.rvo_enabled || k.ahead > 0) return CAVOID_EUNSUPPORTED;
    const int64_t waves = (worlds + k.wpw - 1) / k.wpw;
    if (waves < 1 || waves > 0x7fffffffLL) return CAVOID_EINVAL;
    const size_t lds = crowd_rvo_lds(n, k.tile_rows, io.obs ? io.obs_stride : k.width);
    if (lds > 65536) return CAVOID_EUNSUPPORTED;
    const int rc = n <= 32 ? launch_crowd_rvo_nb<32>(e, mode, k, st, (unsigned)waves, lds, io, s, ev_start, ev_stop)
                           : launch_crowd_rvo_nb<64>(e, mode, k, st, (unsigned)waves, lds, io, s, ev_start, ev_stop);
    if (rc != CAVOID_OK) return rc;
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

int cavoid_launch_crowd_rvo_push(cavoid_env *e, const RolloutCfg &rc, const RolloutState &rs, const RolloutIO &rio, const ActorIO &io, int32_t step,
                                 hipStream_t s) {
    const KCfg &k = e->k;
    const int n = e->cfg.max_agents;
    if (!crowd_form(n) || n < 2 || n > CAVOID_MAX_AGENTS || !k.rvo_enabled || k.ahead > 0) return CAVOID_EUNSUPPORTED;
    const int64_t tiles = (e->W + k.wpw - 1) / k.wpw;
    if (tiles < 1 || tiles > 0x7fffffffLL) return CAVOID_EINVAL;
    const size_t lds = crowd_rvo_lds(n, k.tile_rows, k.width);
    if (lds > 65536) return CAVOID_EUNSUPPORTED;
    if (n <= 32)
        hipLaunchKernelGGL(crowd_rvo_push_kernel<32>, dim3((unsigned)tiles), dim3(128), lds, s, k, e->st, (const PoolRec *)e->pool, rc, rs, rio, io, n, step);
    else
        hipLaunchKernelGGL(crowd_rvo_push_kernel<64>, dim3((unsigned)tiles), dim3(128), lds, s, k, e->st, (const PoolRec *)e->pool, rc, rs, rio, io, n, step);
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}
