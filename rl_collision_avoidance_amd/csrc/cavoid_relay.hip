// cavoid_relay.hip -- env_relay_kernel instantiations (cavoid_relay.hpp): the in-launch step loop of small batches with the
// step cut into roles on several wavefronts of one workgroup per tile.  Own translation unit, compiled with
// -mllvm -disable-machine-licm like the other step-loop units (build.py).
#include "cavoid_launch.hpp"
#include "cavoid_relay.hpp"

using namespace cavoid;

// Beyond the default 64 KiB of dynamic LDS: opted into once per instantiation and DEVICE, at the first launch there that needs it (the
// attribute belongs to the function on the current device).  CAVOID_EUNSUPPORTED when the device does not grant it: the caller then takes
// the two-wavefront pipeline.
constexpr int kRelayMaxDevices = 64;
template <int N>
static int relay_allow_lds() {
    static bool allowed[kRelayMaxDevices] = {};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const bool cached = dev >= 0 && dev < kRelayMaxDevices;
    if (cached && allowed[dev]) return CAVOID_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(env_relay_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRelayLdsLimit) != hipSuccess) {
        (void)hipGetLastError();
        return CAVOID_EUNSUPPORTED;
    }
    if (cached) allowed[dev] = true;
    return CAVOID_OK;
}

// The launch's shape, or why this form does not carry the call.  One function decides for cavoid_launch_relay (which launches it) and for
// cavoid_relay_takes_topup (which the host's look-ahead rule asks BEFORE the refill decision): the two cannot disagree.
struct RelayShape {
    int nc = 0;                 // observation wavefronts
    size_t lds = 0;
    bool topup = false;         // the launch carries the top-up wavefront (KIO::ahead_hi)
};
// want_topup: the caller would like the top-up wavefront (look-ahead rings, not capturing, ...); granted when GEN v1 generates the scenarios
// and two workgroups per CU are still resident with the extra wavefront (the runtime's occupancy calculator, asked once per shape and env)
template <int N>
static int relay_shape_n(cavoid_env *e, int tile_floats, bool want_topup, RelayShape &sh) {
    int nc = e->relay_consumers;
    while (nc > 1 && relay_lds_fixed_bytes<N>() + (size_t)nc * tile_floats * sizeof(float) > kRelayLdsLimit) --nc;
    const size_t lds = relay_lds_fixed_bytes<N>() + (size_t)nc * tile_floats * sizeof(float);
    // one observation wavefront cannot keep up with the loop: the two-wavefront pipeline is the better form then
    if (lds > kRelayLdsLimit || (nc < 2 && e->relay_consumers >= 2)) return CAVOID_EUNSUPPORTED;
    if (lds > 65536) {
        const int rc_opt = relay_allow_lds<N>();
        if (rc_opt != CAVOID_OK) return rc_opt;
    }
    sh.nc = nc;
    sh.lds = lds;
    sh.topup = false;
    if (want_topup && e->k.gen_mode == 0) {
        if (e->relay_topup_nc != nc || e->relay_topup_lds != lds) {
            int blocks = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, reinterpret_cast<const void *>(env_relay_kernel<N>), 64 * (4 + nc), lds) != hipSuccess) {
                (void)hipGetLastError();
                blocks = 0;
            }
            e->relay_topup_nc = nc;
            e->relay_topup_lds = lds;
            e->relay_topup_fits = blocks >= 2;
        }
        sh.topup = e->relay_topup_fits;
    }
    return CAVOID_OK;
}
static int relay_shape(cavoid_env *e, const KIO &io, bool want_topup, RelayShape &sh) {
    const KCfg &k = e->k;
    if (k.rvo_enabled || k.pool_size <= 0 || !io.obs || !io.actions || io.cont) return CAVOID_EUNSUPPORTED;
    if (k.switches & kSwSkipDonePairs) return CAVOID_EUNSUPPORTED;     // (U4 flipped: P would need to know who was frozen; the other loop forms do)
    const int64_t tiles = (e->W + k.wpw - 1) / k.wpw;
    // every tile's workgroup must be resident at once (256 CUs x 2 workgroups): beyond that the tiles run in rounds
    // (measured with 1024 tiles, N = 4: 3.87 vs 2.50 us per step for the two-wavefront pipeline; 1366 tiles, N = 10: 25 vs 8.3)
    if (tiles > 512) return CAVOID_EUNSUPPORTED;
    // wide rows make the observation wavefronts the limit (and N >= 9 spills): measured at 512 tiles, us per step, this kernel /
    // env_pipe_kernel: N = 2 1.42 / 1.97, 3 1.53 / 2.33, 5 1.86 / 2.91, 6 3.11 / 3.29, 8 4.35 / 3.88, 10 8.85 / 4.80
    if (e->cfg.max_agents > kRelayMaxAgents) return CAVOID_EUNSUPPORTED;
    const int row = io.obs_stride;
    const int tile_floats = (k.tile_rows * row + 3) & ~3;
    if (k.tile_rows < k.wpw * e->cfg.max_agents) return CAVOID_EUNSUPPORTED;   // one pass per step only
    return dispatch_n(e->cfg.max_agents, RelayNs{}, [&](auto n) -> int { return relay_shape_n<decltype(n)::value>(e, tile_floats, want_topup, sh); });
}

// the top-up wavefront is asked for where the host's bookkeeping is the whole truth about the rings: not while a stream is capturing and
// not once a hipGraph holds launches of this env (its replays consume episodes the host does not see: cavoid_ahead_prepare)
static bool relay_wants_topup(const cavoid_env *e, hipStream_t s) {
    if (e->ahead_R <= 0 || e->ahead_always || e->k.gen_mode != 0) return false;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s, &cap);
    return cap == hipStreamCaptureStatusNone;
}

bool cavoid_relay_takes_topup(cavoid_env *e, const KIO &io, hipStream_t s) {
    RelayShape sh;
    return relay_wants_topup(e, s) && relay_shape(e, io, true, sh) == CAVOID_OK && sh.topup;
}

int cavoid_launch_relay(cavoid_env *e, const KIO &io, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop) {
    RelayShape sh;
    const int rc_shape = relay_shape(e, io, io.ahead_hi != nullptr, sh);
    if (rc_shape != CAVOID_OK) return rc_shape;
    if ((io.ahead_hi != nullptr) != sh.topup) return CAVOID_EINVAL;   // (the caller decided with cavoid_relay_takes_topup)
    const int64_t tiles = (e->W + e->k.wpw - 1) / e->k.wpw;
    const dim3 grid((unsigned)tiles), block(64 * (3 + sh.nc + (sh.topup ? 1 : 0)));
    const int rc = dispatch_n(e->cfg.max_agents, RelayNs{}, [&](auto n) -> int {
        launch_kernel(env_relay_kernel<decltype(n)::value>, grid, block, sh.lds, s, ev_start, ev_stop, e->k, e->st, e->pool, io);
        return CAVOID_OK;
    });
    if (rc != CAVOID_OK) return rc;
    HIP_TRY(hipGetLastError());
    return note_form(e, CAVOID_OK, CAVOID_FORM_RELAY, sh.nc);       // (the consumer count the launch really uses: cavoid_last_step_form)
}

#ifdef CAVOID_TRACE
int cavoid_debug_trace_relay(unsigned long long *dev_ptr) { return set_trace(dev_ptr); }
#endif
