// cavoid_launch.hpp -- host-side launch plumbing shared by the translation units that instantiate env_kernel:
// cavoid_capi.hip (single-step / reset / observe instantiations) and cavoid_multistep.hip (the instantiations with the
// in-launch step loop, compiled with -mllvm -disable-machine-licm, see build.py).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>

#include "cavoid.h"
#include "cavoid_host.hpp"
#include "cavoid_kernels.hpp"

struct cavoid_env {
    int device = 0;
    int64_t W = 0, A = 0, world_offset = 0;
    cavoid_cfg cfg{};
    cavoid::KCfg k{};
    cavoid::KState st{};
    cavoid::PoolRec *pool = nullptr;     // pre-generated scenarios (GEN v1 worlds 0..P-1, episode 0), 64-byte records
    uint32_t *pool_episode = nullptr;   // [P] scratch episode counters for the fill launch
    int64_t pool_size = 0;
    int ahead_R = 0;                    // scenario look-ahead (cfg.gen_lookahead): `pool` is then every world's ring of R records, filled by ahead_fill_kernel
    uint32_t *ahead_hi[2] = {nullptr, nullptr};   // [W] highest episode in each world's ring (0xFFFFFFFF: none): a refill reads [ahead_cur], writes the other
    int ahead_cur = 0;
    int ahead_budget = 0;               // restarts per world the ring is still guaranteed to cover without a refill
    bool ahead_primed = false;          // the rings have been filled once for the current seed / episodes
    bool ahead_always = false;          // a hipGraph holding stepping launches of this env exists: replays consume episodes the host does not see,
                                        // so from then on every launch carries the refill (a no-op when nothing is missing)
    int64_t ahead_refills = 0;          // ahead_fill_kernel launches so far (cavoid_ahead_info)
    int relay_topup_nc = -1;            // env_relay_kernel's top-up wavefront: the shape (consumers, dynamic LDS) the occupancy calculator was last
    size_t relay_topup_lds = 0;         // asked about, and whether two workgroups per CU are resident with it
    bool relay_topup_fits = false;
    int relay_tiles = 0;                // env_relay_kernel's tiles per workgroup: 0 = where it pays (cavoid_relay.hip, relay_duo_wanted), 1 / 2 forced (CAVOID_RELAY_TILES)
    int relay_duo_nc = -1;              // ... the two-tile shape (consumers, dynamic LDS) the device was last asked about, and whether one workgroup of it
    size_t relay_duo_lds = 0;           // is resident: bit 0 without, bit 1 with the top-up wavefronts
    int relay_duo_fit = 0;
    int relay_cus = 0;                  // the device's CU count, once asked (relay_duo_wanted)
    void *slab = nullptr;
    void *pool_slab = nullptr;
    double *d_actions = nullptr;
    int waves_per_block = 4;
    int grid = 0;
    int pipeline = 2;            // latency mode, multi-step launches: 2 = env_relay_kernel (roles on 5-7 wavefronts per tile), 1 = env_pipe_kernel
                                 // (two wavefronts per tile), 0 = one wavefront per tile (CAVOID_PIPELINE)
    int relay_consumers = 0;     // observation wavefronts per tile of env_relay_kernel (CAVOID_RELAY_CONSUMERS, 1..4); 0: the launcher's default
                                 // (3 with one tile per workgroup, 4 with two: cavoid_relay.hip)
    int latency_mode = 0;        // small batch: multi-step launches keep the next pool record in registers (MODE_STEP_AUTORESET_PF)
    int quad = -1;               // one-step auto-reset launches with four cooperating wavefronts per tile (env_quad_kernel): -1 = where it pays
                                 // (<= 512 tiles), 0 / 1 = never / wherever it can run (CAVOID_QUAD)
    int prefetch_single = 0;     // ... and single-step launches too (CAVOID_PREFETCH_POOL=1; costs 64 B of reads per agent-step)
    int last_form = CAVOID_FORM_NONE;   // what the last successful stepping call launched (cavoid_last_step_form): set by the dispatcher that launched
    int last_relay_consumers = 0;       // ... and, for CAVOID_FORM_RELAY, the consumer count it used
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};


namespace cavoid {

// ---- the N-dispatch: the agents per world each launch form is instantiated for, written once per form ----------------------------------
template <int... Ns>
struct NList {};
#ifdef CAVOID_DEV_ONLY_N   /* development builds: instantiate a few sizes only (compile time) */
#ifndef CAVOID_DEV_ENV_NS  /* ... these, unless the build names its own (-DCAVOID_DEV_ENV_NS=3,4,5: build.build_plain_dist) */
#define CAVOID_DEV_ENV_NS 4, 10
#endif
#ifndef CAVOID_DEV_RELAY_NS
#define CAVOID_DEV_RELAY_NS 4
#endif
using EnvNs = NList<CAVOID_DEV_ENV_NS>;     // env_kernel, env_pipe_kernel, ahead_fill_kernel, actor_kernel, step_push_kernel
using RelayNs = NList<CAVOID_DEV_RELAY_NS>; // env_relay_kernel
using QuadNs = NList<4>;                    // env_quad_kernel
#else
using EnvNs = NList<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>;
using RelayNs = NList<1, 2, 3, 4, 5, 6>;    // 1 .. kRelayMaxAgents (cavoid_relay.hpp)
using QuadNs = NList<2, 3, 4, 5, 6, 10>;
#endif

// the agent counts the crowd form (cavoid_crowd.hip) carries: kTileMaxAgents + 1 .. CAVOID_MAX_AGENTS.  The development build
// -DCAVOID_DEV_CROWD_FROM_N=k routes every N >= k there (the drift test holds it bitwise to the tile forms at small N).
#ifdef CAVOID_DEV_CROWD_FROM_N
constexpr int kCrowdFromN = CAVOID_DEV_CROWD_FROM_N;
#else
constexpr int kCrowdFromN = kTileMaxAgents + 1;
#endif
static inline bool crowd_form(int max_agents) { return max_agents >= kCrowdFromN; }

// f(std::integral_constant<int, N>{}) for the N of the list equal to n (decltype(arg)::value in f); CAVOID_EUNSUPPORTED for an n the list does not hold
template <int... Ns, class F>
static inline int dispatch_n(int n, NList<Ns...>, F &&f) {
    int rc = CAVOID_EUNSUPPORTED;
    (void)((n == Ns ? (rc = f(std::integral_constant<int, Ns>{}), true) : false) || ...);
    return rc;
}

// one launch: the extension launch when the caller times it with events, else the plain launch (capturable into a hipGraph)
template <class K, class... Args>
static inline void launch_kernel(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop,
                                 const Args &...args) {
    if (ev_start || ev_stop) hipExtLaunchKernelGGL(kernel, grid, block, lds, s, ev_start, ev_stop, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
}

#ifdef CAVOID_TRACE
// development build only: point THIS translation unit's copy of the phase-stamp pointer g_trace somewhere (every env unit has its own;
// cavoid_debug_trace sets them all)
static inline int set_trace(unsigned long long *dev_ptr) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &dev_ptr, sizeof(dev_ptr)));
    return CAVOID_OK;
}
#endif

// the dispatchers' bookkeeping for cavoid_last_step_form: a launch that succeeded records its form
static inline int note_form(cavoid_env *e, int rc, int form, int relay_consumers = 0) {
    if (rc == CAVOID_OK) {
        e->last_form = form;
        e->last_relay_consumers = relay_consumers;
    }
    return rc;
}

template <int MODE, bool RVO = false>
static inline int launch_on(cavoid_env *e, const KCfg &k, const KState &st, int grid_x, const KIO &io, hipStream_t s,
                     hipEvent_t ev_start, hipEvent_t ev_stop) {
    const dim3 grid(grid_x), block(64 * e->waves_per_block);
    // dynamic LDS: the action table + per wavefront the staging arrays and an obs tile of this launch's row width
    const int row = io.obs ? io.obs_stride : k.width;
    int tile = (k.tile_rows * row + 3) & ~3;
    if (tile < k.park_floats) tile = k.park_floats;
    const size_t lds = (size_t)(lds_floats_block() + e->waves_per_block * (lds_floats_fixed(e->cfg.max_agents) + k.rvo_lds_floats + tile)) * sizeof(float);
    const int rc = dispatch_n(e->cfg.max_agents, EnvNs{}, [&](auto n) -> int {
        launch_kernel(env_kernel<decltype(n)::value, MODE, RVO>, grid, block, lds, s, ev_start, ev_stop, k, st, e->pool, io);
        return CAVOID_OK;
    });
    if (rc != CAVOID_OK) return rc;
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}


// The two-wavefront pipelined step loop (env_pipe_kernel): one 128-thread workgroup per tile.  Returns CAVOID_EUNSUPPORTED when
// its LDS (two staging + two hand-over buffers, the obs tile, the ORCA scratch) does not fit 64 KiB: the caller then takes
// the single-wavefront loop.
template <bool RVO>
static inline int launch_pipe(cavoid_env *e, const KIO &io, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop) {
    const KCfg &k = e->k;
    if (!io.obs) return CAVOID_EUNSUPPORTED;               // (the consumer wavefront IS the observation: env_kernel guards a null obs)
    if (k.gen_mode == 1 && k.pool_size <= 0) return CAVOID_EUNSUPPORTED;   // (box scenarios generated inside the step: env_kernel's restart)
    const int64_t tiles = (e->W + k.wpw - 1) / k.wpw;
    // it pays while the chip can hold both wavefronts of every tile at <= 2 per SIMD (1024 SIMDs): measured at N = 4,
    // 32-step launches: 512 / 1024 tiles 2.50 vs 3.02 / 3.06 us per step, 2048 tiles 5.05 vs 3.75; N = 10, 1366 tiles 9.4 vs 8.2
    if (tiles > 1024) return CAVOID_EUNSUPPORTED;
    const int row = io.obs ? io.obs_stride : k.width;
    int tile = (k.tile_rows * row + 3) & ~3;
    if (tile < k.park_floats) tile = k.park_floats;
    const size_t tail = (size_t)(tile + k.rvo_lds_floats) * sizeof(float);
    const dim3 grid((unsigned)tiles), block(128);
    const int rc = dispatch_n(e->cfg.max_agents, EnvNs{}, [&](auto n) -> int {
        constexpr int N = decltype(n)::value;
        const size_t lds = pipe_lds_fixed_bytes<N>() + tail;
        if (lds > 65536) return CAVOID_EUNSUPPORTED;
        launch_kernel(env_pipe_kernel<N, RVO>, grid, block, lds, s, ev_start, ev_stop, k, e->st, e->pool, io);
        return CAVOID_OK;
    });
    if (rc != CAVOID_OK) return rc;
    HIP_TRY(hipGetLastError());
    return CAVOID_OK;
}

}  // namespace cavoid

// scenario look-ahead: make sure every world's ring covers the restarts `n_steps` more steps can bring (a no-op without look-ahead);
// CAVOID_EUNSUPPORTED when n_steps + 1 > R (cavoid_capi.hip)
// timed_start (may be null): a start event the caller wants recorded where the launch's work begins -- when a refill is launched it is recorded
// in front of THAT kernel and *timed_start is set to null (the stepping kernel behind it then records only its stop event), so that a timed
// launch includes its refill (cavoid_step_autoreset_n_timed)
// relay_topup: the launch behind it is env_relay_kernel WITH its top-up wavefront (cavoid_relay_takes_topup said so): it needs the rings to
// cover n_steps episodes only, regenerates what earlier launches consumed itself and leaves a budget of R - n_steps
int cavoid_ahead_prepare(cavoid_env *e, int32_t n_steps, hipStream_t s, hipEvent_t *timed_start = nullptr, bool relay_topup = false);
void cavoid_ahead_consumed(cavoid_env *e, int32_t n_steps, bool relay_topup = false);     // call after the stepping launch that cavoid_ahead_prepare(n_steps) preceded
// env_relay_kernel (cavoid_relay.hip): CAVOID_EUNSUPPORTED when the batch is too large for it or its LDS does not fit
int cavoid_launch_relay(cavoid_env *e, const cavoid::KIO &io, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop);
// the multi-step launch of this call tries env_relay_kernel first (cavoid_launch_multistep's order, written once)
static inline bool relay_form_first(const cavoid_env *e, const cavoid::KIO &io, bool prefetch) {
    return !cavoid::crowd_form(e->cfg.max_agents) && !e->k.rvo_enabled && !(e->k.gen_mode == 1 && e->k.pool_size <= 0) && prefetch && e->pipeline >= 2 &&
           !io.cont;
}
// ... and cavoid_launch_relay will carry it with the top-up wavefront, given io.ahead_hi: the refusals of cavoid_launch_relay, look-ahead
// rings generated by GEN v1, no stream capture now or earlier, two workgroups per CU resident with the extra wavefront
bool cavoid_relay_takes_topup(cavoid_env *e, const cavoid::KIO &io, hipStream_t s);
// multi-step auto-reset launch (cavoid_multistep.hip): prefetch != 0 -> MODE_STEP_AUTORESET_PF, else MODE_STEP_AUTORESET_N
// env_quad_kernel (cavoid_quad.hip): CAVOID_EUNSUPPORTED when the configuration or the launch is not one it carries
int cavoid_launch_quad(cavoid_env *e, const cavoid::KIO &io, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop);
int cavoid_launch_multistep(cavoid_env *e, const cavoid::KIO &io, bool prefetch, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop);
// any stepping mode for an env with rvo_enabled (cavoid_rvo.hip: the instantiations that carry the ORCA policy)
int cavoid_launch_rvo(cavoid_env *e, int mode, const cavoid::KIO &io, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop);
// any mode of an env of more than kTileMaxAgents agents per world (cavoid_crowd.hip): `worlds` of k (the env's, or the pool's for the
// pool fill) in ceil(worlds / k.wpw) one-wavefront workgroups; CAVOID_EUNSUPPORTED for a configuration the form does not carry
int cavoid_launch_crowd(cavoid_env *e, int mode, const cavoid::KCfg &k, const cavoid::KState &st, int64_t worlds, const cavoid::KIO &io,
                        hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop);
// the stepping modes of such an env with rvo_enabled (cavoid_crowd_rvo.hip: the kernels that carry the wave-cooperative ORCA solve);
// cavoid_launch_crowd routes there
int cavoid_launch_crowd_rvo(cavoid_env *e, int mode, const cavoid::KCfg &k, const cavoid::KState &st, int64_t worlds, const cavoid::KIO &io,
                            hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop);
// what a stepping launch of a crowd env reports to cavoid_last_step_form
static inline int crowd_step_form(const cavoid_env *e) { return e->k.rvo_enabled ? CAVOID_FORM_CROWD_RVO : CAVOID_FORM_CROWD; }
#ifdef CAVOID_TRACE
// development build only: cavoid::set_trace of the env units other than cavoid_capi.hip (cavoid_debug_trace calls them all)
int cavoid_debug_trace_multistep(unsigned long long *dev_ptr);
int cavoid_debug_trace_rvo(unsigned long long *dev_ptr);
int cavoid_debug_trace_relay(unsigned long long *dev_ptr);
int cavoid_debug_trace_quad(unsigned long long *dev_ptr);
#endif
