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
constexpr int kRelaySoloConsumers = 3, kRelayDuoConsumers = 4;   // consumers per tile where CAVOID_RELAY_CONSUMERS names none: one / two tiles per workgroup
template <int N, int TPW = 1>
static int relay_allow_lds() {
    static bool allowed[kRelayMaxDevices] = {};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const bool cached = dev >= 0 && dev < kRelayMaxDevices;
    if (cached && allowed[dev]) return CAVOID_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(env_relay_kernel<N, TPW>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(TPW * kRelayLdsLimit)) != hipSuccess) {
        (void)hipGetLastError();
        return CAVOID_EUNSUPPORTED;
    }
    if (cached) allowed[dev] = true;
    return CAVOID_OK;
}

// The launch's shape, or why this form does not carry the call.  One function decides for cavoid_launch_relay (which launches it) and for
// cavoid_relay_takes_topup (which the host's look-ahead rule asks BEFORE the refill decision): the two cannot disagree.
struct RelayShape {
    int nc = 0;                 // observation wavefronts per tile
    size_t lds = 0;             // the workgroup's dynamic LDS (TPW = 2: both tiles' regions)
    bool topup = false;         // the launch carries the top-up wavefront (KIO::ahead_hi)
    int tpw = 1;                // tiles per workgroup
};
// Two tiles per workgroup (cavoid_relay.hpp, relay_duo_slot), with FOUR consumers per tile unless CAVOID_RELAY_CONSUMERS names a count:
// by default where it was measured to win (profiles/relay_duo_timing.txt) -- N = 4, and so many tiles that two of them share EVERY CU
// anyway, i.e. the workgroups of two tiles leave no CU idle (8192 worlds: 512 tiles on 256 CUs).  With fewer tiles one tile per workgroup
// spreads over more CUs and keeps its three consumers.  CAVOID_RELAY_TILES=1|2 (read at cavoid_create) forces the answer for every tile
// count and every N <= kRelayDuoMaxN.  What the device has to grant is asked in relay_duo_fits.
static bool relay_duo_wanted(cavoid_env *e, int n, int64_t tiles) {
    if (n > kRelayDuoMaxN || e->relay_tiles == 1) return false;
    if (e->relay_tiles == 2) return true;
    if (n != 4) return false;
    if (e->relay_cus <= 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
            (void)hipGetLastError();
            return false;
        }
        e->relay_cus = cus;
    }
    return (tiles + 1) / 2 >= e->relay_cus;
}
// ... the instantiation runs without scratch, the doubled LDS is within the device's per-workgroup limit (opted into), and the runtime's
// occupancy calculator holds one workgroup of that shape resident -- with the top-up's two wavefronts when they are wanted, else without
// them (the answer per env and shape is kept)
template <int N>
static bool relay_duo_fits(cavoid_env *e, int nc, size_t lds, bool want_topup, bool &topup) {
    if constexpr (N > kRelayDuoMaxN) return false;
    else {
        if (e->relay_duo_nc != nc || e->relay_duo_lds != lds) {
            e->relay_duo_nc = nc;
            e->relay_duo_lds = lds;
            e->relay_duo_fit = 0;
            const void *fn = reinterpret_cast<const void *>(env_relay_kernel<N, 2>);
            hipFuncAttributes fa{};
            int lim = 0, dev = 0;
            bool ok = hipGetDevice(&dev) == hipSuccess && hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.localSizeBytes == 0 &&
                      hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess;
            if (ok && lds > (size_t)lim) {                  // (beyond the default limit: the opt-in decides, then the occupancy calculator)
                int optin = 0;
                if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) == hipSuccess && optin > 0) ok = lds <= (size_t)optin;
            }
            ok = ok && (lds <= 65536 || relay_allow_lds<N, 2>() == CAVOID_OK);
            for (int t = 1; ok && t >= 0; --t) {
                int blocks = 0;
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, 64 * relay_duo_waves(nc, t), lds) == hipSuccess && blocks >= 1) e->relay_duo_fit |= 1 << t;
            }
            (void)hipGetLastError();
        }
        topup = want_topup && (e->relay_duo_fit & 2) != 0;
        return (e->relay_duo_fit & (topup ? 2 : 1)) != 0;
    }
}
// want_topup: the caller would like the top-up wavefront (look-ahead rings, not capturing, ...); granted when GEN v1 generates the scenarios
// and two workgroups per CU are still resident with the extra wavefront (the runtime's occupancy calculator, asked once per shape and env)
template <int N>
static int relay_shape_n(cavoid_env *e, int tile_floats, bool want_topup, RelayShape &sh) {
    // the consumers a tile gets: the count asked for (CAVOID_RELAY_CONSUMERS; else `dflt`), lowered until the tile's region fits its half of a CU's LDS
    auto consumers = [&](int dflt, int &asked) {
        int nc = asked = e->relay_consumers > 0 ? e->relay_consumers : dflt;
        while (nc > 1 && relay_region_bytes(relay_lds_fixed_bytes<N>(), nc, tile_floats) > kRelayLdsLimit) --nc;
        return nc;
    };
    sh.topup = false;
    const int64_t tiles = (e->W + e->k.wpw - 1) / e->k.wpw;
    if (relay_duo_wanted(e, N, tiles)) {
        int asked = 0;
        const int nc2 = consumers(kRelayDuoConsumers, asked);
        const size_t lds2 = relay_lds_bytes(2, relay_lds_fixed_bytes<N>(), nc2, tile_floats);
        bool topup2 = false;
        if (lds2 <= 2 * kRelayLdsLimit && !(nc2 < 2 && asked >= 2) && relay_duo_fits<N>(e, nc2, lds2, want_topup && e->k.gen_mode == 0, topup2)) {
            sh.nc = nc2;
            sh.lds = lds2;
            sh.topup = topup2;
            sh.tpw = 2;
            return CAVOID_OK;
        }
    }
    int asked = 0;
    const int nc = consumers(kRelaySoloConsumers, asked);
    const size_t lds = relay_region_bytes(relay_lds_fixed_bytes<N>(), nc, tile_floats);
    // one observation wavefront cannot keep up with the loop: the two-wavefront pipeline is the better form then
    if (lds > kRelayLdsLimit || (nc < 2 && asked >= 2)) return CAVOID_EUNSUPPORTED;
    if (lds > 65536) {
        const int rc_opt = relay_allow_lds<N>();
        if (rc_opt != CAVOID_OK) return rc_opt;
    }
    sh.nc = nc;
    sh.lds = lds;
    sh.tpw = 1;
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

static int g_relay_last_tiles = 0;      // tiles per workgroup of this process's last relay launch (cavoid_relay_last_tiles, for the tests)

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
    const dim3 grid((unsigned)((tiles + sh.tpw - 1) / sh.tpw)), block(64 * sh.tpw * (3 + sh.nc + (sh.topup ? 1 : 0)));
    const int rc = dispatch_n(e->cfg.max_agents, RelayNs{}, [&](auto n) -> int {
        constexpr int N = decltype(n)::value;
        if constexpr (N <= kRelayDuoMaxN) {
            if (sh.tpw == 2) {
                launch_kernel(env_relay_kernel<N, 2>, grid, block, sh.lds, s, ev_start, ev_stop, e->k, e->st, e->pool, io);
                return CAVOID_OK;
            }
        }
        launch_kernel(env_relay_kernel<N>, grid, block, sh.lds, s, ev_start, ev_stop, e->k, e->st, e->pool, io);
        return CAVOID_OK;
    });
    if (rc != CAVOID_OK) return rc;
    HIP_TRY(hipGetLastError());
    g_relay_last_tiles = sh.tpw;
    return note_form(e, CAVOID_OK, CAVOID_FORM_RELAY, sh.nc);       // (the consumer count the launch really uses: cavoid_last_step_form)
}

// The TPW = 2 role table and LDS layout as the kernel and the launcher compute them, for tests/test_relay_duo_host.py (host only, no device):
// wavefront wv of a workgroup with nc consumers per tile -> (tile << 4) | role, -1 beyond the workgroup's wavefronts; and the bytes of a
// launch's dynamic LDS (what = 2), of one tile's region (what = 3) and the offset of the region of tile `what` = 0 | 1, at N agents per world.
extern "C" int32_t cavoid_relay_duo_slot(int32_t wv, int32_t nc, int32_t topup, int32_t mate) {
    if (wv < 0 || nc < 1 || nc > kRelayMaxConsumers || wv >= relay_duo_waves(nc, topup)) return -1;
    return relay_duo_slot(wv, nc, mate < 0 ? CAVOID_RELAY_DUO_MATE : mate);
}
// ... and the tiles per workgroup of the last relay launch this process made (0: none yet): tests/test_gpu_relay_duo.py proves the form ran
extern "C" int32_t cavoid_relay_last_tiles(void) { return g_relay_last_tiles; }
extern "C" int64_t cavoid_relay_lds_layout(int32_t n, int32_t tpw, int32_t nc, int32_t tile_floats, int32_t what) {
    int64_t r = -1;
    (void)dispatch_n(n, NList<1, 2, 3, 4, 5, 6>{}, [&](auto nn) -> int {
        const size_t fixed = relay_lds_fixed_bytes<decltype(nn)::value>();
        r = what == 2 ? (int64_t)relay_lds_bytes(tpw, fixed, nc, tile_floats) : what == 3 ? (int64_t)relay_region_bytes(fixed, nc, tile_floats)
                                                                                          : (int64_t)relay_region_offset(what, fixed, nc, tile_floats);
        return CAVOID_OK;
    });
    return r;
}

#ifdef CAVOID_TRACE
int cavoid_debug_trace_relay(unsigned long long *dev_ptr) { return set_trace(dev_ptr); }
#endif
