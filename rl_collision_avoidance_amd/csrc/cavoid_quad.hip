// cavoid_quad.hip -- env_quad_kernel instantiations (cavoid_quad.hpp): one auto-reset step per launch with four cooperating wavefronts per
// tile -- the closed-loop `env.step` of small batches, where a step is one wavefront's dependent chain per tile and most SIMDs idle.
#include <cstdlib>

#include "cavoid_launch.hpp"
#include "cavoid_quad.hpp"

using namespace cavoid;

int cavoid_launch_quad(cavoid_env *e, const KIO &io, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop) {
    const KCfg &k = e->k;
    if (e->quad == 0) return CAVOID_EUNSUPPORTED;          // CAVOID_QUAD=0
    if (k.rvo_enabled || (k.gen_mode == 1 && k.pool_size <= 0) || !io.obs || !io.actions || io.cont) return CAVOID_EUNSUPPORTED;
    if (k.dynamics == CAVOID_DYN_HOLONOMIC) return CAVOID_EUNSUPPORTED;
    const int64_t tiles = (e->W + k.wpw - 1) / k.wpw;
    // it pays while every tile's four wavefronts are resident at <= 2 per SIMD (1024 SIMDs): beyond that the single-wavefront form's
    // throughput wins (CAVOID_QUAD=1 forces it for A/B runs)
    if (e->quad < 0 && tiles > 512) return CAVOID_EUNSUPPORTED;
    if (k.tile_rows < k.wpw * e->cfg.max_agents) return CAVOID_EUNSUPPORTED;   // one pass per step only
    const int row = io.obs_stride;
    const int tile_floats = (k.tile_rows * row + 3) & ~3;
    const dim3 grid((unsigned)tiles), block(256);
    const int rc = dispatch_n(e->cfg.max_agents, QuadNs{}, [&](auto n) -> int {
        constexpr int N = decltype(n)::value;
        const size_t lds = quad_lds_bytes<N>(tile_floats);
        if (lds > 65536) return CAVOID_EUNSUPPORTED;
        launch_kernel(env_quad_kernel<N>, grid, block, lds, s, ev_start, ev_stop, k, e->st, e->pool, io);
        return CAVOID_OK;
    });
    if (rc != CAVOID_OK) return rc;
    HIP_TRY(hipGetLastError());
    return note_form(e, CAVOID_OK, CAVOID_FORM_QUAD);
}

#ifdef CAVOID_TRACE
int cavoid_debug_trace_quad(unsigned long long *dev_ptr) { return set_trace(dev_ptr); }
#endif
