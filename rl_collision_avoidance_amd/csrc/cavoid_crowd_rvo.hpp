// cavoid_crowd_rvo.hpp -- ORCA (policy 3) agents in the crowd step form: the wavefront solves ONE agent's programme at a time, one
// lane per constraint line (CAVOID_FORM_CROWD_RVO, cfg.rvo_enabled = CAVOID_RVO_WAVE).
//
// The tile forms' rvo_action (cavoid_kernels.hpp) keeps two sets of N-1 lines of four doubles PER LANE in wave-private LDS: 4 KiB per
// wavefront and neighbour, 258 KB at N = 64 where a workgroup may ask for 64 KiB and the crowd form already uses 58 KB.  Here a lane is
// an agent, so the lanes of a world ARE the neighbours of any of its agents: for the host agent h the lane of neighbour j builds the
// half-plane of j (crowd_orca_line: rvo_action's loop body, statement for statement), the lines of one host go to LDS once (2 x (N-1) x 32 B, in the sort
// keys' region, idle until the pair pass), and the two programmes' inner loops -- over the lines in front of line k -- become one lane
// per earlier line and a wavefront reduction.  The walk over k stays serial and wave-uniform, as does the running optimum.
//
// Bit-identical to rvo_action, not close to it (tests/test_gpu_crowd_rvo.py holds the development build that routes every N here to
// the tile forms byte for byte): see the argument at the reductions in crowd_lp_on_line.
//
// rvo_action's line body, preferred velocity and tail are COPIED here (crowd_orca_line, crowd_orca_preferred, crowd_orca_action; each marked),
// as crowd_tile copies env_tile: split into functions that rvo_action calls too, they gave the 123 ORCA-carrying kernels of the tile
// forms another instruction stream (commutative float64 operands swapped: the same values, not the same code), and those kernels keep
// theirs.  The bitwise test is the guard on the copies.
#pragma once
#include "cavoid_kernels.hpp"

namespace cavoid {

// the lines of the host being solved: field f of line k of set s at mem[(s * 4 + f) * no + k] (field-major: lane k reads line k, the
// wavefront reads 64 consecutive doubles).  Set 0: the ORCA lines in agent-index order; set 1: least-penetration's projected lines.
struct CrowdLines {
    double *mem; int no;
    __device__ __forceinline__ Line get(int set, int k) const {
        const double *p = mem + set * 4 * no + k;
        return Line{p[0], p[no], p[2 * no], p[3 * no]};
    }
    __device__ __forceinline__ void put(int set, int k, const Line &l) const {
        double *p = mem + set * 4 * no + k;
        p[0] = l.px; p[no] = l.py; p[2 * no] = l.dx; p[3 * no] = l.dy;
    }
};
__host__ __device__ constexpr int crowd_rvo_line_floats(int n) { return 2 * 4 * (n - 1) * 2; }

// ---- mirrors rvo_action's loop body: the half-plane (ORCA line) the agent at relative position (rpx, rpy), seen at relative velocity
// (rvx, rvy) = host - other, imposes on a host of radius `radius` and last velocity (hvx, hvy); rjf: the other agent's radius ----------
__device__ __forceinline__ Line crowd_orca_line(const KCfg &c, float radius, float rjf, double rpx, double rpy, double rvx, double rvy, double hvx,
                                                double hvy) {
    const double dist_sq = rpx * rpx + rpy * rpy;
    const double comb = c.cold->rvo_radius_scale * (double)radius + c.cold->rvo_radius_scale * (double)rjf, comb_sq = comb * comb;
    double dx, dy, ucx, ucy;
    if (dist_sq > comb_sq) {
        const double wx = rvx - c.cold->rvo_inv_horizon * rpx, wy = rvy - c.cold->rvo_inv_horizon * rpy;
        const double w_sq = wx * wx + wy * wy, dot1 = wx * rpx + wy * rpy;
        if (dot1 < 0.0 && dot1 * dot1 > comb_sq * w_sq) {
            const double w_len = sqrt(w_sq), ux = wx / w_len, uy = wy / w_len, scale = comb * c.cold->rvo_inv_horizon - w_len;
            dx = uy; dy = -ux; ucx = scale * ux; ucy = scale * uy;
        } else {
            const double leg = sqrt(dist_sq - comb_sq);
            if (det2(rpx, rpy, wx, wy) > 0.0) { dx = (rpx * leg - rpy * comb) / dist_sq; dy = (rpx * comb + rpy * leg) / dist_sq; }
            else { dx = -(rpx * leg + rpy * comb) / dist_sq; dy = -(-rpx * comb + rpy * leg) / dist_sq; }
            const double dot2 = rvx * dx + rvy * dy;
            ucx = dot2 * dx - rvx; ucy = dot2 * dy - rvy;
        }
    } else {
        const double inv_dt = 1.0 / c.dt, wx = rvx - inv_dt * rpx, wy = rvy - inv_dt * rpy;
        const double w_len = sqrt(wx * wx + wy * wy), ux = wx / w_len, uy = wy / w_len, scale = comb * inv_dt - w_len;
        dx = uy; dy = -ux; ucx = scale * ux; ucy = scale * uy;
    }
    return Line{hvx + c.cold->rvo_collab * ucx, hvy + c.cold->rvo_collab * ucy, dx, dy};
}
// ---- mirrors rvo_action: the velocity the programmes prefer -- straight at the goal at the preferred speed ----------------------------
__device__ __forceinline__ void crowd_orca_preferred(const Agent &a, double &ox, double &oy) {
    const double gx = (double)a.gx - a.px, gy = (double)a.gy - a.py, gn = sqrt(gx * gx + gy * gy);
    const double scale = gn > 0.0 ? (double)a.pref / gn : 0.0;
    ox = scale * gx; oy = scale * gy;
}
// ---- mirrors rvo_action's tail: [speed, delta_heading] of the solved velocity; turns beyond rvo_max_dh are clipped and taken standing still
__device__ __forceinline__ void crowd_orca_action(const KCfg &c, const Agent &a, double vx, double vy, double &a0, double &a1) {
    double speed = sqrt(vx * vx + vy * vy);
    double delta = 0.0;
    if (speed > 0.0) {
        delta = atan2(vy, vx) - a.heading;
        while (delta >= kPi) delta -= 2.0 * kPi;
        while (delta < -kPi) delta += 2.0 * kPi;
        delta = wrap_closed_fixup(delta, c.switches);
    }
    if (fabs(delta) > c.cold->rvo_max_dh) { delta = copysign(c.cold->rvo_max_dh, delta); speed = 0.0; }
    a0 = speed; a1 = delta;
}

// a condition every lane computed from the same values, as a scalar: the branches of the programmes stay wave-uniform
__device__ __forceinline__ bool wave_same(bool b) { return __ballot(b) != 0ull; }
__device__ __forceinline__ double lane_read(double v, int src) {             // src wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float lane_read(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
// min / max over the lanes that hold lines (0 .. NB-2), every lane receiving lane 0's result
template <int NB>
__device__ __forceinline__ double wave_fmin(double v) {
#pragma unroll
    for (int off = 1; off < NB; off <<= 1) v = fmin(v, __shfl_xor(v, off));
    return lane_read(v, 0);
}
template <int NB>
__device__ __forceinline__ double wave_fmax(double v) {
#pragma unroll
    for (int off = 1; off < NB; off <<= 1) v = fmax(v, __shfl_xor(v, off));
    return lane_read(v, 0);
}

// lp_on_line with its loop over the lines i < k spread over the lanes: lane i holds line i.
template <int NB>
__device__ __forceinline__ bool crowd_lp_on_line(const CrowdLines &L, int set, int k, double radius, double ox, double oy, bool direction_opt, int lane,
                                                 double &x, double &y) {
    const Line l = L.get(set, k);
    const double dot = l.px * l.dx + l.py * l.dy, disc = dot * dot + radius * radius - (l.px * l.px + l.py * l.py);
    if (wave_same(disc < 0.0)) return false;
    const double root = sqrt(disc);
    double t_lo = -dot - root, t_hi = -dot + root;
    const bool mine = lane < k;
    const Line o = L.get(set, mine ? lane : 0);
    const double den = det2(l.dx, l.dy, o.dx, o.dy), num = det2(o.dx, o.dy, l.px - o.px, l.py - o.py);
    const bool parallel = fabs(den) <= kRvoEps, bounds = mine && !parallel;
    const double t = num / den;
    // Why the reductions give lp_on_line's result to the bit.  (1) t_hi is the fmin of its start value and the t of every line with
    // den >= 0, t_lo the fmax of its start value and the t of the others: every t is finite (|den| > kRvoEps), fmin / fmax of finite
    // values do not depend on the order (v_min_f64 / v_max_f64 order -0 below +0), and the start value enters last here and first
    // there.  (2) The serial loop returns false as soon as t_lo > t_hi; t_lo only rises and t_hi only falls, so that happens at some
    // prefix exactly when it holds at the end.  (3) Its other `return false` -- a parallel line with num < 0 -- is any-lane here; the
    // function has no effect before it returns false, so which test fires first does not matter.  (4) Every lane's den, num and t are
    // lp_on_line's statements on the same operands, compiled with the same flags (-ffp-contract=off).
    t_hi = fmin(t_hi, wave_fmin<NB>(bounds && den >= 0.0 ? t : INFINITY));
    t_lo = fmax(t_lo, wave_fmax<NB>(bounds && !(den >= 0.0) ? t : -INFINITY));
    if (__ballot(mine && parallel && num < 0.0) != 0ull || wave_same(t_lo > t_hi)) return false;
    double tt;
    if (direction_opt) tt = (ox * l.dx + oy * l.dy > 0.0) ? t_hi : t_lo;
    else { tt = l.dx * (ox - l.px) + l.dy * (oy - l.py); tt = tt < t_lo ? t_lo : (tt > t_hi ? t_hi : tt); }
    x = l.px + tt * l.dx; y = l.py + tt * l.dy;
    return true;
}

// lp_plane: the walk over k serial, every lane carrying the same optimum
template <int NB>
__device__ __forceinline__ int crowd_lp_plane(const CrowdLines &L, int set, int m, double radius, double ox, double oy, bool direction_opt, int lane,
                                              double &x, double &y) {
    if (direction_opt) { x = ox * radius; y = oy * radius; }
    else if (ox * ox + oy * oy > radius * radius) { const double nn = sqrt(ox * ox + oy * oy); x = ox / nn * radius; y = oy / nn * radius; }
    else { x = ox; y = oy; }
#pragma unroll 1
    for (int k = 0; k < m; ++k) {
        const Line l = L.get(set, k);
        if (wave_same(det2(l.dx, l.dy, l.px - x, l.py - y) > 0.0)) {
            double nx, ny;
            if (!crowd_lp_on_line<NB>(L, set, k, radius, ox, oy, direction_opt, lane, nx, ny)) return k;
            x = nx; y = ny;
        }
    }
    return m;
}

// lp_least_penetration: the projected set of line k built one lane per j < k; its `continue` (a parallel line pointing the same
// way) becomes a compaction that keeps the order -- slot = the number of kept lines below j
template <int NB>
__device__ __forceinline__ void crowd_lp_least_penetration(const CrowdLines &L, int m, int begin, double radius, int lane, double &x, double &y) {
    double distance = 0.0;
#pragma unroll 1
    for (int k = begin; k < m; ++k) {
        const Line l = L.get(0, k);
        if (wave_same(det2(l.dx, l.dy, l.px - x, l.py - y) > distance)) {
            const bool mine = lane < k;
            const Line o = L.get(0, mine ? lane : 0);
            const double den = det2(l.dx, l.dy, o.dx, o.dy);
            double nx, ny;
            bool keep = mine;
            if (fabs(den) <= kRvoEps) {
                if (l.dx * o.dx + l.dy * o.dy > 0.0) keep = false;
                nx = 0.5 * (l.px + o.px); ny = 0.5 * (l.py + o.py);
            } else {
                const double t = det2(o.dx, o.dy, l.px - o.px, l.py - o.py) / den;
                nx = l.px + t * l.dx; ny = l.py + t * l.dy;
            }
            const double fx = o.dx - l.dx, fy = o.dy - l.dy, fn = sqrt(fx * fx + fy * fy);
            const uint64_t kept = __ballot(keep);
            if (keep) L.put(1, __popcll(kept & ((1ull << lane) - 1ull)), Line{nx, ny, fx / fn, fy / fn});
            const int np = __popcll(kept);
            wave_lds_sync();
            if (crowd_lp_plane<NB>(L, 1, np, radius, -l.dy, l.dx, true, lane, nx, ny) >= np) { x = nx; y = ny; }
            distance = det2(l.dx, l.dy, l.px - x, l.py - y);
            wave_lds_sync();                                     // the next k overwrites set 1
        }
    }
}

// a0 / a1 of every lane with a running ORCA agent (`orca`).  lds_* hold the PRE-move state of the wavefront's agents as rvo_action
// reads it (positions, last float64 velocities, radii; radius < 0: absent); n agents per world, a lane's world begins at lane `base`.
template <int NB>
__device__ __forceinline__ void crowd_rvo_actions(const KCfg &c, const Agent &a, bool orca, int n, int lane, const double *lds_px, const double *lds_py,
                                                  const double *lds_vx, const double *lds_vy, const float *lds_r, double *line_mem, double &a0,
                                                  double &a1) {
    const CrowdLines L{line_mem, n - 1};
    const double my_px = lds_px[lane], my_py = lds_py[lane], my_vx = lds_vx[lane], my_vy = lds_vy[lane];
    const float my_r = lds_r[lane];
    double pref_x = 0.0, pref_y = 0.0, vx = 0.0, vy = 0.0;
    if (orca) crowd_orca_preferred(a, pref_x, pref_y);
#pragma unroll 1
    for (uint64_t todo = __ballot(orca); todo != 0ull; todo &= todo - 1ull) {
        const int h = __builtin_amdgcn_readfirstlane((int)__ffsll((unsigned long long)todo) - 1);      // the host agent's lane
        const int hb = h - h % n;                                                                       // ... and its world's first lane
        // ---- lines: lane j of the host's world builds the half-plane of neighbour j -- rvo_action's loop body ------------------
        const double hpx = lds_px[h], hpy = lds_py[h], hvx = lds_vx[h], hvy = lds_vy[h];
        const float hr = lds_r[h];
        const bool line = lane >= hb && lane < hb + n && lane != h && !(my_r < 0.0f);
        const uint64_t lines = __ballot(line);
        const int m = __popcll(lines);
        if (line) {
            const double rpx = my_px - hpx, rpy = my_py - hpy, rvx = hvx - my_vx, rvy = hvy - my_vy;
            // compact slot: the present agents of the world below this one, the host excluded -- agent-index order, on which the
            // programme's result depends
            L.put(0, __popcll(lines & ((1ull << lane) - 1ull)), crowd_orca_line(c, hr, my_r, rpx, rpy, rvx, rvy, hvx, hvy));
        }
        wave_lds_sync();
        // ---- programme ----------------------------------------------------------------------------------------------------------
        const double radius = (double)lane_read(a.pref, h), ox = lane_read(pref_x, h), oy = lane_read(pref_y, h);
        double sx, sy;
        const int fail = crowd_lp_plane<NB>(L, 0, m, radius, ox, oy, false, lane, sx, sy);
        if (fail < m) crowd_lp_least_penetration<NB>(L, m, fail, radius, lane, sx, sy);
        if (lane == h) { vx = sx; vy = sy; }
        wave_lds_sync();                                         // the next host overwrites the lines
    }
    // ---- action: rvo_action's tail, by the ORCA lanes alone -----------------------------------------------------------------------
    if (orca) crowd_orca_action(c, a, vx, vy, a0, a1);
}

}  // namespace cavoid
