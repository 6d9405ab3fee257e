// cavoid_crowd.hpp -- the crowd step form (CAVOID_FORM_CROWD): worlds of 17..64 agents, the agent count taken at run time.
//
// Mapping: one lane per agent, a wavefront (one 64-thread workgroup) owns floor(64/N) whole worlds -- three of 17..21 agents,
// two of 22..32, one of 33..64.  What the tile forms keep in per-lane register arrays sized by N lives in wave-private LDS here:
//   recs   StageRec[64]            the staged post-move records (one per lane, read at base + j by the world's other lanes)
//   vel    double[2][64]           float64 velocities for the time-to-impact order
//   gen    4 x double[64] + float[64]  the box generator's placements (GEN v2 generated in the kernel)
//   gaps   float[N-1][64]          the observation gap of each neighbour, field-major (lane-private column)
//   pos    uint8[N-1][64]          the rank of each neighbour
//   keys   uint64[N-1][64]         the 63-bit sort keys; once the ranks are made the same region is the obs tile (rows go out in
//                                  passes of c.tile_rows rows: a 64 x 449-float N = 64 tile would not fit)
// Semantics are env_tile's (cavoid_kernels.hpp): E4 decode, E5 dynamics, E6 pairs, E7/E8 reward and done, the restart and the E9
// rows are the same statements in the same order; each copy is marked with the env_tile block it mirrors.  The neighbour order is
// the tile forms' order: the same Key, the same tie rule (two equal keys send the whole wavefront to the exact path), the same
// exact path.  Ranking counts, for every neighbour, the keys below its own (see crowd_rank).
#pragma once
#include "cavoid_kernels.hpp"
#include "cavoid_crowd_rvo.hpp"

namespace cavoid {

// per-wavefront LDS of the crowd kernel, in floats: recs, vel, gen, gaps, pos, then the keys / obs tile region
__host__ __device__ constexpr int crowd_lds_fixed_floats(int n) {
    return 64 * (int)(sizeof(StageRec) / sizeof(float)) + 64 * 2 * 2 + lds_floats_scratch() + (n - 1) * 64 + (n - 1) * 16;
}
__host__ __device__ constexpr int crowd_key_floats(int n) { return (n - 1) * 64 * 2; }
__host__ __device__ inline int crowd_tile_floats(int n, int tile_rows, int ostride) {
    const int need = (tile_rows * ostride + 3) & ~3;
    return need > crowd_key_floats(n) ? need : crowd_key_floats(n);
}
__host__ __device__ inline int crowd_wave_floats(int n, int tile_rows, int ostride) {
    return crowd_lds_fixed_floats(n) + crowd_tile_floats(n, tile_rows, ostride);
}

// Scenario of (global world gw, episode ep) for a world of n agents -- new_episode<N> with the agent count at run time
template <int NB>
__device__ __forceinline__ void crowd_new_episode(const KCfg &c, const PoolRec *pool, uint32_t gw, uint32_t ep, int i, int n, Agent &a) {
    if (c.pool_size > 0) {
        load_pool(pool, (int64_t)pool_index(c, gw, ep) * n + i, a);
    } else {
        generate_agent<NB>(c, gw, ep, i, a);
    }
}

// E6 of one lane against the n-1 others of its world, in ring order (o -> agent (i + 1 + o) mod n): pair_pass_impl's statements
// with the keys and gaps written to LDS (its PARK form) and the valid / frozen masks 64 bits wide.
template <bool SW>
__device__ __forceinline__ void crowd_pair_pass_impl(const KCfg &c, const Agent &a, const Ego &e, bool present, const StageRec *recs, int i,
                                                     int base, int n, uint64_t *keys, float *gaps, int lane, uint64_t &valid, bool &hit,
                                                     double &min_gap, uint64_t frozen_w) {
    const double ri = (double)a.radius;
    valid = 0ull;
    hit = false;
    min_gap = INFINITY;
#pragma unroll 2
    for (int o = 0; o < n - 1; ++o) {
        // ---- mirrors pair_pass_impl's `one(o)` -------------------------------------------------------------------------------
        const int jj = other_index(i, o, n);
        const StageRec *qr = recs + base + jj;
        const OtherState q{qr->px, qr->py, qr->vxf, qr->vyf, qr->r};
        const float rjf = q.r;
        const double rx = q.px - a.px, ry = q.py - a.py;
#if defined(CAVOID_DEV_ULP_FAULT) && CAVOID_DEV_ULP_FAULT == 1
        const double d = sqrt_dist2((double)((float)rx * (float)rx) + ry * ry);
#else
        const double d = sqrt_dist2(rx * rx + ry * ry);
#endif
        const bool other = present && (rjf >= 0.0f);
        bool collides = other;
        if (SW) collides = other && ((frozen_w >> jj) & 1ull) == 0ull && ((frozen_w >> i) & 1ull) == 0ull;
        const double gap_c = d - (ri + (double)rjf);
        min_gap = collides ? fmin(min_gap, gap_c) : min_gap;
        hit = hit || (collides && gap_c <= c.collision_dist);
        const bool seen = other && !(d > c.horizon);
        valid |= seen ? (1ull << o) : 0ull;
        const double gap_o = d - ri - (double)rjf;
#if defined(CAVOID_DEV_ULP_FAULT) && CAVOID_DEV_ULP_FAULT == 3
        uint32_t hi = kKeyBias - (uint32_t)(int)rintf((float)gap_o * 100.0f);
#else
        uint32_t hi = kKeyBias - (uint32_t)(int)rint(gap_o * 100.0);
#endif
        uint32_t lo = orderable((float)(ry * e.tx - rx * e.ty));
        if (SW) {
            if (c.switches & kSwIndexTie) lo = (uint32_t)jj;
            if (c.switches & kSwExactGap) { lo = 0u; hi = 0x7FFFFFFEu - (orderable((float)gap_o) >> 1); }
        }
        hi = seen ? hi : kKeySentinel + (uint32_t)o;
        keys[o * 64 + lane] = ((uint64_t)hi << 32) | lo;
        gaps[o * 64 + lane] = (float)gap_o;
    }
}
__device__ __forceinline__ void crowd_pair_pass(const KCfg &c, const Agent &a, const Ego &e, bool present, const StageRec *recs, int i, int base,
                                                int n, uint64_t *keys, float *gaps, int lane, uint64_t &valid, bool &hit, double &min_gap,
                                                uint64_t frozen_w = 0ull) {
    if (CAVOID_RARE(c.switches != 0u))
        crowd_pair_pass_impl<true>(c, a, e, present, recs, i, base, n, keys, gaps, lane, valid, hit, min_gap, frozen_w);
    else
        crowd_pair_pass_impl<false>(c, a, e, present, recs, i, base, n, keys, gaps, lane, valid, hit, min_gap, 0ull);
}

// The ranking: pos[o] = the number of keys below key o -- for distinct keys exactly tournament()'s result (its pos[o] counts
// the later neighbours at or below and the earlier ones strictly below), and two equal keys get the same count, so
// "some position taken twice" is tournament()'s `differ == 0`: the caller then ranks the exact way.
// Counting over keys in LDS, B of them in registers at a time: each key is read ONCE per block of B (ceil((N-1)/B) (N-1) LDS
// reads instead of (N-1)^2) and a compare is a 64-bit subtraction and the borrow's add -- about 4 vector instructions per ordered
// pair, (N-1)^2 pairs.  The tournament's 5 instructions per unordered pair ((N-1)(N-2)/2 pairs) need every key in registers at
// once (126 VGPRs at N = 64, compile-time indexed, plus the ranks) or a read-modify-write of the ranks in LDS per pair block;
// the counting form keeps 3 B + a few registers live and needs no compile-time N.
// ASC (closest_first's re-rank): the bucket half flipped, as tournament<..., true>; MASKED: neighbours outside `mask` become the
// slot's sentinel (k2 of assemble_obs).
template <int B, bool ASC, bool MASKED>
__device__ __forceinline__ uint64_t crowd_key(const uint64_t *keys, int o, int lane, uint64_t mask) {
    uint64_t v = keys[o * 64 + lane];
    uint32_t hi = (uint32_t)(v >> 32);
    const uint32_t lo = (uint32_t)v;
    if (MASKED) hi = ((mask >> o) & 1ull) ? hi : kKeySentinel + (uint32_t)o;
    if (ASC) hi = key_is_sentinel(hi) ? hi : 2u * kKeyBias - hi;
    return ((uint64_t)hi << 32) | lo;
}
template <int B, bool ASC, bool MASKED>
__device__ __forceinline__ bool crowd_rank(const uint64_t *keys, uint8_t *pos, int no, int lane, uint64_t mask) {
    uint64_t taken = 0ull;
    for (int o0 = 0; o0 < no; o0 += B) {                       // (wave-uniform)
        uint64_t kb[B];
        int cnt[B];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            kb[b] = o0 + b < no ? crowd_key<B, ASC, MASKED>(keys, o0 + b, lane, mask) : 0ull;
            cnt[b] = 0;
        }
#pragma unroll 2
        for (int q = 0; q < no; ++q) {
            const uint64_t kq = crowd_key<B, ASC, MASKED>(keys, q, lane, mask);
#pragma unroll
            for (int b = 0; b < B; ++b) cnt[b] += (int)((kq - kb[b]) >> 63);   // both < 2^63: bit 63 <=> kq < kb
        }
#pragma unroll
        for (int b = 0; b < B; ++b)
            if (o0 + b < no) {
                pos[(o0 + b) * 64 + lane] = (uint8_t)cnt[b];
                taken |= 1ull << cnt[b];
            }
    }
    return __popcll(taken) != no;
}

// env_tile for a world of n agents (17..64; any n >= 2 in the development build that routes every N here).  NB: the bucket
// (32 or 64) -- the generator's round count and the ranking's register block.  out (may be null): the step's results of this lane's
// agent, handed over in registers where env_tile hands them over (crowd_push_kernel, cavoid_crowd_push.hpp).
// RVO: the instantiation can drive policy-3 (ORCA) agents -- the wavefront solves one agent's programme at a time
// (cavoid_crowd_rvo.hpp).  Instantiations of their own (crowd_rvo_kernel, cavoid_crowd_rvo.hip), as for env_tile: the programmes
// inlined into the step cost every other configuration registers for code it never runs.
template <int NB, int MODE, bool RVO = false>
__device__ __forceinline__ void crowd_tile(const KCfg &c, const KState &s, const PoolRec *pool, const KIO &io, const int n, double *lds_tab,
                                           float *wbase, const int lane, const int64_t wave, StepOut *out = nullptr) {
    constexpr bool kAuto = MODE == MODE_STEP_AUTORESET_N;
    constexpr bool kLoop = MODE == MODE_STEP_AUTORESET_N;
    constexpr bool kStepping = MODE == MODE_STEP || kAuto;
    constexpr int kB = NB > 32 ? 16 : 8;                  // the ranking's register block
    const int width = c.width, ostride = io.obs ? io.obs_stride : width;
    const int no = n - 1;
    StageRec *recs = reinterpret_cast<StageRec *>(wbase);
    double *vx64 = reinterpret_cast<double *>(recs + 64), *vy64 = vx64 + 64;
    double *lds_px = vy64 + 64;
    double *lds_py = lds_px + 64, *lds_gx = lds_py + 64, *lds_gy = lds_gx + 64;
    float *lds_r = reinterpret_cast<float *>(lds_gy + 64);
    float *gaps = lds_r + 64;
    uint8_t *pos = reinterpret_cast<uint8_t *>(gaps + no * 64);
    float *tile = reinterpret_cast<float *>(pos + no * 64);          // (no * 64 bytes: a multiple of 16)
    uint64_t *keys = reinterpret_cast<uint64_t *>(tile);

    // ---- mirrors env_tile: lane mapping, loads ----------------------------------------------------------------------------------
    const int wpw = c.wpw, lanes_used = wpw * n;
    const int64_t w0 = wave * wpw;
    const int lw = lane / n, i = lane - lw * n;
    const int64_t w = w0 + lw;
    const bool active = lane < lanes_used && w < c.num_worlds;
    const int base = lane < lanes_used ? lw * n : 0;
    const int64_t a_idx = w * n + i;
    const bool packed = io.packed != 0;
    int64_t worlds_here = c.num_worlds - w0;
    if (worlds_here > wpw) worlds_here = wpw;
    if (worlds_here < 0) worlds_here = 0;

    double tab_v = 0.0;
    const bool use_table = kStepping && io.actions != nullptr;
    if (use_table && lane < 2 * c.num_actions) tab_v = c.action_table[lane];

    Agent a;
    a.px = a.py = a.heading = a.t_rem = a.vx = a.vy = 0.0;
    a.gx = a.gy = a.radius = a.pref = a.speed = 0.0f;
    a.flags = 0u;
    uint32_t episode = 0u;
    bool fresh = false;
    int act_next = 0;
    float c1_next = 0.f;
    if (active) {
        if (MODE == MODE_RESET) {
            fresh = io.mask == nullptr || io.mask[w] != 0;
            episode = s.episode[w] + (fresh ? 1u : 0u);
        } else if (kAuto) {
            episode = s.episode[w];
        }
        if (!fresh) {
            load_agent(s, a_idx, a);
            if (!kStepping || RVO) a.speed = s.speed[a_idx];   // (ORCA agents read the others' last velocities)
        }
        if (kStepping) {
            if (io.cont) { act_next = __float_as_int(io.cont[2 * a_idx]); c1_next = io.cont[2 * a_idx + 1]; }
            else act_next = io.actions[a_idx];
        }
    }
    if (use_table) lds_tab[lane] = tab_v;
    const bool present_first = active && (a.flags & CAVOID_F_PRESENT);

    if (MODE == MODE_RESET) {
        if (io.pool_out) episode = c.pool_epoch;
        if (c.gen_mode == 1 && c.pool_size == 0)
            generate_world_v2<NB>(c, (uint32_t)(c.world_offset + w), episode, i, base, lane, fresh, lds_px, lds_py, lds_gx, lds_gy, lds_r, a);
        else if (fresh) crowd_new_episode<NB>(c, pool, (uint32_t)(c.world_offset + w), episode, i, n, a);
    }
    if (MODE == MODE_OBSERVE || MODE == MODE_RESET) {
        double sn, cs;
        sincos_bounded(a.heading, &sn, &cs);
        a.vx = (double)a.speed * cs;
        a.vy = (double)a.speed * sn;
    }

    const int n_steps = kLoop ? io.n_steps : 1;
    bool restarted_any = false, moved_any = false;
    const int lane0 = lane, i0 = i, base0 = base;
    const int64_t a_idx0 = a_idx;
    auto write_back = [&]() {
        // ---- mirrors env_tile's write_back --------------------------------------------------------------------------------------
        if (restarted_any) {
            store_agent(s, a_idx0, a);
            if (i0 == 0) s.episode[w] = episode;
        } else if (present_first) {
            if (moved_any) {
                s.px[a_idx0] = a.px; s.py[a_idx0] = a.py; s.heading[a_idx0] = a.heading; s.t_rem[a_idx0] = a.t_rem;
            }
            s.speed[a_idx0] = a.speed;
            s.flags[a_idx0] = a.flags;
        }
    };
    for (int t = 0; t < n_steps; ++t) {
    int lane = lane0, i = i0, base = base0;
    int64_t a_idx = a_idx0;
    if (kLoop) asm volatile("" : "+v"(lane), "+v"(i), "+v"(base), "+v"(a_idx));
    const uint32_t flags_in = a.flags;
    const bool present_in = active && (flags_in & CAVOID_F_PRESENT);
    const bool done_in = (flags_in & CAVOID_F_DONE_MASK) != 0u;
    int act = act_next;
    const float c1 = c1_next;
    if (kLoop && t + 1 < n_steps && active) {
        if (CAVOID_RARE(io.cont != nullptr)) {
            const float *cn = io.cont + (int64_t)(t + 1) * io.action_stride + 2 * a_idx;
            act_next = __float_as_int(cn[0]); c1_next = cn[1];
        } else act_next = io.actions[(int64_t)(t + 1) * io.action_stride + a_idx];
    }
    const int64_t slot_w = kLoop ? (int64_t)t * io.out_step_stride : 0;

    if (kStepping) {
        // ---- mirrors env_tile: E4 decode ---------------------------------------------------------------------------------------
        wave_lds_sync();
        const uint32_t pol = (flags_in >> CAVOID_F_POLICY_SHIFT) & CAVOID_F_POLICY_MASK;
        double a0 = 0.0, a1 = 0.0;
        if (io.cont) { a0 = (double)__int_as_float(act); a1 = (double)c1; }
        else {
            act = act < 0 ? 0 : (act >= c.num_actions ? c.num_actions - 1 : act);
            a0 = (double)a.pref * lds_tab[2 * act];
            a1 = lds_tab[2 * act + 1];
        }
        if (CAVOID_RARE(__ballot(present_in && !done_in && pol != 0u) != 0ull)) {
            if (pol == 1u) { a0 = 0.0; a1 = 0.0; }
            if (pol == 2u) {
                const Ego e0 = ego_frame_exact(c, a);
                a0 = (double)a.pref;
                a1 = -e0.heading_ego;
            }
        }
        const bool orca = present_in && !done_in && pol == 3u;
        if (RVO && CAVOID_RARE(__ballot(orca) != 0ull)) {        // ORCA agents in this tile
            // ---- mirrors env_tile: the PRE-move state of every agent, in the box generator's scratch (idle here) ---------------
            double sn, cs;
            sincos_bounded(a.heading, &sn, &cs);
            lds_px[lane] = a.px; lds_py[lane] = a.py;
            lds_gx[lane] = present_in ? (double)a.speed * cs : 0.0;
            lds_gy[lane] = present_in ? (double)a.speed * sn : 0.0;
            lds_r[lane] = present_in ? a.radius : -1.0f;
            wave_lds_sync();
            // the lines of the agent being solved lie in the keys region: idle until the pair pass
            crowd_rvo_actions<NB>(c, a, orca, n, lane, lds_px, lds_py, lds_gx, lds_gy, lds_r, reinterpret_cast<double *>(keys), a0, a1);
            wave_lds_sync();
        }
        if (c.actions_fp32) { a0 = (double)(float)a0; a1 = (double)(float)a1; }
        // ---- mirrors env_tile: E5 dynamics -------------------------------------------------------------------------------------
        const bool moving = present_in && !done_in;
        moved_any = moved_any || moving;
        double npx, npy, nh, nvx, nvy, nsp;
        if (CAVOID_RARE(c.dynamics == CAVOID_DYN_HOLONOMIC)) {
            nsp = sqrt(a0 * a0 + a1 * a1);
            nh = nsp > 0.0 ? atan2(a1, a0) : a.heading;
            npx = a.px + a0 * c.dt; npy = a.py + a1 * c.dt;
            nvx = a0; nvy = a1;
        } else {
            double dh = a1;
            if (CAVOID_RARE(c.dynamics == CAVOID_DYN_UNICYCLE_MAX_TURN)) {
                const double rate = fmin(fmax(dh / c.dt, -c.cold->max_turn_rate), c.cold->max_turn_rate);
                dh = rate * c.dt;
            }
            nh = wrap_angle(dh + a.heading, c.switches);
            double sn = 0.0, cs = 1.0;
            sincos_bounded(nh, &sn, &cs);
#if defined(CAVOID_DEV_ULP_FAULT) && CAVOID_DEV_ULP_FAULT == 2
            npx = __builtin_fma(a0 * cs, c.dt, a.px); npy = __builtin_fma(a0 * sn, c.dt, a.py);
#else
            npx = a.px + a0 * cs * c.dt; npy = a.py + a0 * sn * c.dt;
#endif
            nvx = a0 * cs; nvy = a0 * sn; nsp = a0;
        }
        a.px = moving ? npx : a.px; a.py = moving ? npy : a.py; a.heading = moving ? nh : a.heading;
        a.vx = moving ? nvx : 0.0; a.vy = moving ? nvy : 0.0; a.speed = moving ? (float)nsp : 0.0f;
        if (present_in && done_in) {
            if (flags_in & CAVOID_F_AT_GOAL) a.flags |= CAVOID_F_WAS_AT_GOAL;
            if (flags_in & CAVOID_F_IN_COLL) a.flags |= CAVOID_F_WAS_IN_COLL;
        }
        if (moving) {
            const double dx = a.px - (double)a.gx, dy = a.py - (double)a.gy;
            if (dx * dx + dy * dy <= c.near_goal_sq) a.flags |= CAVOID_F_AT_GOAL;
            a.t_rem -= c.dt;
            if (c.timeout_enabled && a.t_rem <= 0.0) a.flags |= CAVOID_F_RAN_OUT;
        }
    }

    // ---- mirrors env_tile: stage post-move state, E6 pair pass ------------------------------------------------------------------
    bool present = active && (a.flags & CAVOID_F_PRESENT);
    const bool tti = c.sort_method == CAVOID_SORT_TIME_TO_IMPACT;
    auto stage_self = [&](bool is_present) {
        recs[lane] = StageRec{a.px, a.py, (float)a.vx, (float)a.vy, is_present ? a.radius : -1.0f, 0.0f};
        if (CAVOID_RARE(tti)) { vx64[lane] = a.vx; vy64[lane] = a.vy; }
    };
    stage_self(present);
    wave_lds_sync();
    Ego e = ego_frame_obs(c, a);
    uint64_t valid;
    bool hit;
    double min_gap;
    uint64_t frozen_w = 0ull;
    const uint64_t wbits = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
    if (kStepping && CAVOID_RARE(c.switches & kSwSkipDonePairs))
        frozen_w = (__ballot(present_in && done_in) >> base) & wbits;
    crowd_pair_pass(c, a, e, present, recs, i, base, n, keys, gaps, lane, valid, hit, min_gap, frozen_w);

    float rew_f = 0.0f, done_f = (present && (a.flags & CAVOID_F_DONE_MASK) == 0u) ? 0.0f : 1.0f;
    if (kStepping) {
        // ---- mirrors env_tile: E7 rewards, E8 done -----------------------------------------------------------------------------
        double r = 0.0;
        bool done = true;
        if (present) {
            r = c.r_step;
            if (a.flags & CAVOID_F_AT_GOAL) { if (!(a.flags & CAVOID_F_WAS_AT_GOAL)) r = c.r_goal; }
            else if (!(a.flags & CAVOID_F_WAS_IN_COLL)) {
                if (hit) { r = c.r_coll; a.flags |= CAVOID_F_IN_COLL; }
                else if (min_gap <= c.close_range) r = c.r_close + c.close_slope * min_gap;
            }
            r = fmin(fmax(r, c.clip_lo), c.clip_hi);
            done = (a.flags & CAVOID_F_DONE_MASK) != 0u;
        }
        const unsigned long long running = __ballot(present && ((a.flags & CAVOID_F_LEARNING) || c.evaluate_mode) && !done);
        const unsigned long long wmask = wbits << base;
        const bool game_over = (running & wmask) == 0ull;
        rew_f = (float)r;
        done_f = done ? 1.0f : 0.0f;
        if (out) { out->reward = rew_f; out->done = done; out->game_over = game_over; out->flags = a.flags; }
        if (active) {
            if (!packed) {
                io.rew[slot_w * n + a_idx] = rew_f;
                io.done[slot_w * n + a_idx] = done ? 1 : 0;
            }
            if (i == 0) io.game_over[slot_w + w] = game_over ? 1 : 0;
        }
        if (kAuto) {
            // ---- mirrors env_tile: the restart ----------------------------------------------------------------------------------
            const bool restart = active && game_over;
            if (CAVOID_RARE(__ballot(restart) != 0ull)) {
                wave_lds_sync();
                if (restart) { episode += 1u; restarted_any = true; }
                const bool box_in_step = c.gen_mode == 1 && c.pool_size == 0;     // (the generator's scratch is its own region here)
                if (box_in_step)
                    generate_world_v2<NB>(c, (uint32_t)(c.world_offset + w), episode, i, base, lane, restart, lds_px, lds_py, lds_gx, lds_gy,
                                          lds_r, a);
                if (restart) {
                    if (!box_in_step) crowd_new_episode<NB>(c, pool, (uint32_t)(c.world_offset + w), episode, i, n, a);
                    present = (a.flags & CAVOID_F_PRESENT) != 0u;
                    stage_self(present);
                }
                wave_lds_sync();
                if (restart) {
                    e = ego_frame_obs(c, a);
                    bool hit2;
                    double gap2;
                    crowd_pair_pass(c, a, e, present, recs, i, base, n, keys, gaps, lane, valid, hit2, gap2);
                }
            }
        }
    }

    if (out) out->learning_next = active && (a.flags & CAVOID_F_PRESENT) != 0u && (a.flags & CAVOID_F_LEARNING) != 0u;
    if (kStepping && !kLoop) write_back();
    // ---- mirrors env_tile's E9 (assemble_obs): ranks, then the rows in passes of c.tile_rows ----------------------------------------
    if (io.obs) {
        wave_lds_sync();
        const int M = c.max_other;
        const double ri = (double)a.radius;
        auto criteria = [&](int o, double &g, double &l, double &tt, int &jj) {
            jj = other_index(i, o, n);
            const StageRec *qr = recs + base + jj;
            const double rj = (double)qr->r;
            const double rx = qr->px - a.px, ry = qr->py - a.py;
            const double gap = sqrt_dist2(rx * rx + ry * ry) - ri - rj;
            g = (c.switches & kSwExactGap) ? gap : rint(gap * 100.0);
            l = (c.switches & kSwIndexTie) ? 0.0 : ry * e.tx - rx * e.ty;
            tt = 0.0;
            if (tti) tt = time_to_impact(rx, ry, a.vx - vx64[base + jj], a.vy - vy64[base + jj], ri + rj);
        };
        // assemble_obs's rank_exact, the ranks written to `pos`
        auto rank_exact = [&](uint64_t among, bool near_first, bool use_tti) {
            const int n_among = __popcll(among);
#pragma unroll 1
            for (int p = 0; p < no; ++p) {
                double gp, lp, tp;
                int jp;
                criteria(p, gp, lp, tp, jp);
                int before = 0;
#pragma unroll 1
                for (int q = 0; q < no; ++q) {
                    double gq, lq, tq;
                    int jq;
                    criteria(q, gq, lq, tq, jq);
                    const bool tie_break = (lq < lp) || (lq == lp && jq < jp);
                    const bool by_gap = near_first ? (gq < gp) || (gq == gp && tie_break) : (gq > gp) || (gq == gp && tie_break);
                    const bool q_first = use_tti ? (tq > tp) || (tq == tp && by_gap) : by_gap;
                    before += (q != p && ((among >> q) & 1ull) && q_first) ? 1 : 0;
                }
                const bool member = (among >> p) & 1ull;
                pos[p * 64 + lane] = (uint8_t)(member ? before : n_among + __popcll(~among & ((1ull << p) - 1ull)));
            }
        };
        const int m = __popcll(valid);
        const int first = m > M ? m - M : 0;
        const int kept = m - first;
        bool generic = tti;
        if (!generic) {
            const bool tie = crowd_rank<kB, false, false>(keys, pos, no, lane, 0ull);
            generic = __ballot(tie) != 0ull;
        }
        if (CAVOID_RARE(generic)) rank_exact(valid, false, tti);
        uint64_t keep = 0ull;
        for (int o = 0; o < no; ++o) keep |= (((valid >> o) & 1ull) && pos[o * 64 + lane] >= first) ? (1ull << o) : 0ull;
        int slot_bias = first;
        if (CAVOID_RARE(c.sort_method == CAVOID_SORT_CLOSEST_FIRST)) {
            slot_bias = 0;
            const bool tie = crowd_rank<kB, true, true>(keys, pos, no, lane, keep);
            if (CAVOID_RARE(__ballot(tie) != 0ull)) rank_exact(keep, true, false);
        }
        wave_lds_sync();                                         // the keys region becomes the obs tile
        const bool present_o = active && (a.flags & CAVOID_F_PRESENT);
        const float pxf = (float)e.prll_x, pyf = (float)e.prll_y;
        const int rows_active = (int)worlds_here * n, rpp = c.tile_rows;
        float *obs_dst = io.obs + (slot_w + w0) * n * ostride;
        const bool stream_out = kLoop ? io.out_step_stride != 0 : c.stream_obs != 0;
        for (int p0 = 0; p0 < rows_active; p0 += rpp) {
            if (active && lane >= p0 && lane < p0 + rpp) {
                float *row = tile + (lane - p0) * ostride;
                write_row_head(row, a, e, present_o, kept, kept, M, packed, width, rew_f, done_f);
                for (int o = 0; o < no; ++o) {
                    if (!((keep >> o) & 1ull)) continue;
                    const StageRec *qr = recs + base + other_index(i, o, n);
                    const OtherState q{qr->px, qr->py, qr->vxf, qr->vyf, qr->r};
                    float f[kFeat];
                    neighbour_features(e, pxf, pyf, q.px - a.px, q.py - a.py, q, f);
                    float *dst = row + 6 + 7 * ((int)pos[o * 64 + lane] - slot_bias);
                    dst[0] = f[0]; dst[1] = f[1]; dst[2] = f[2]; dst[3] = f[3]; dst[4] = f[4]; dst[5] = a.radius + f[4]; dst[6] = gaps[o * 64 + lane];
                }
            }
            wave_lds_sync();
            const int rows_here = rows_active - p0 < rpp ? rows_active - p0 : rpp;
            if (stream_out) flush_tile<8, true>(tile, obs_dst + (int64_t)p0 * ostride, rows_here * ostride, lane, 64);
            else flush_tile<8>(tile, obs_dst + (int64_t)p0 * ostride, rows_here * ostride, lane, 64);
            wave_lds_sync();                                     // the next pass overwrites the tile
        }
    }
    if (kLoop && n_steps > 1) wave_lds_sync();
    }   // step loop

    if (kStepping && kLoop) write_back();
    if (MODE == MODE_RESET) {
        // ---- mirrors env_tile: the reset's stores ---------------------------------------------------------------------------------
        if (fresh && io.pool_out) {
            PoolRec r;
            r.px = a.px; r.py = a.py; r.heading = a.heading; r.t_rem = a.t_rem;
            r.gx = a.gx; r.gy = a.gy; r.radius = a.radius; r.pref = a.pref;
            r.flags = a.flags; r.pad[0] = r.pad[1] = r.pad[2] = 0u;
            io.pool_out[a_idx] = r;
        } else if (fresh) {
            store_agent(s, a_idx, a);
            if (i == 0) s.episode[w] = episode;
        }
    }
}

// one wavefront per workgroup: the LDS a wavefront needs grows with N (19 KB at N = 17 .. 58 KB at N = 64), and a workgroup of
// one wavefront lets the CU pack as many as its 160 KiB hold
template <int NB, int MODE>
__global__ void __launch_bounds__(64) crowd_kernel(const KCfg c, const KState s, const PoolRec *pool, const KIO io, const int n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *lds_tab = reinterpret_cast<double *>(smem);
    float *wbase = reinterpret_cast<float *>(smem) + lds_floats_block();
    crowd_tile<NB, MODE>(c, s, pool, io, n, lds_tab, wbase, (int)threadIdx.x, (int64_t)blockIdx.x);
}
// ... and the stepping modes of an env whose worlds may hold ORCA agents (cavoid_crowd_rvo.hip)
template <int NB, int MODE>
__global__ void __launch_bounds__(64) crowd_rvo_kernel(const KCfg c, const KState s, const PoolRec *pool, const KIO io, const int n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *lds_tab = reinterpret_cast<double *>(smem);
    float *wbase = reinterpret_cast<float *>(smem) + lds_floats_block();
    crowd_tile<NB, MODE, true>(c, s, pool, io, n, lds_tab, wbase, (int)threadIdx.x, (int64_t)blockIdx.x);
}

}  // namespace cavoid
