"""Shared cases of the tests that hold the ORCA policy (policy 3) to the oracle branch by branch, after the pattern of tests/tie_regimes.py.
A plain module: tests/test_orca_regimes_host.py (CPU: both oracles, the traces, the flips, the straddles) and
tests/test_gpu_orca_regimes.py (tile and crowd forms) build the SAME batches from it.

Generator scenarios reach the rare branches of the linear programmes -- a parallel line, the mid-point line, a failed projected
programme, an exact zero of a determinant -- a handful of times in a hundred thousand programmes or never, so the worlds here are
placed by hand and pushed with set_state.  oracle/cavoid_oracle.py names every decision of orca_lines, _lp_on_line, _lp_plane,
_lp_least_penetration and rvo_action and passes it through a hook: `trace` records the host's decisions, `flip` returns the
opposite at one of them.

BRANCH cases (groups "default" and "off": the four ORCA fields off their defaults) take the named decision with a margin: the
trace survives +-1e-12 on every coordinate, and flipping the decision moves the host's action by more than 1e-3.  They were found
by a seeded search over hosts at the origin with 2 to 5 neighbours on a 1/8 m grid, half of them then moved off the grid by
irrational offsets (`inexact`); the table below is its result, written out, and the host test proves every claim again.  Every
world holds a halted learner far away whose time budget ends the world one step after the decision: what follows a placed
decision is of no interest and may be a tie.
EXACT cases (group "exact": dt 0.25, horizon 4, radius scale 1, collab 0.5) are made of exactly representable numbers with every
mover on heading exactly 0, so that the deciding quantity is computed without rounding on both sides: below / at / above triples
around dist_sq == comb_sq, det2(rp, w) == 0, dot1 == 0 and num == 0 of two coincident lines.  The displacement of below / above is
the smallest number of ulps of one coordinate that changes the computed quantity (a denormal shift underflows in the products).
Every agent of an exact world has a budget of one dt: the world is over after the step that meets the decision.

Layout: a case is a host (ORCA) and its neighbours in line order.  It is placed three times -- the host as agent 0 (the deciding
lines in the lowest slots), as the agent behind its neighbours (a middle agent; far static agents fill the world up to N present
agents behind it) and as the last present agent behind the fillers and the neighbours (the deciding lines in the highest slots) --
and every fourth case leaves the rest of its first placement absent.  The three placements of case c sit in worlds 6 c + (c + v) % 3
(v = 0, 1, 2), generator worlds in 6 c + 3 .. 6 c + 5: over the cases every placement is the first, second and third world of a
wavefront of three (N = 17 .. 21) and the first and second of a wavefront of two (N = 22 .. 32)."""
import collections
import math

import numpy as np

from oracle import c_oracle as co
from oracle import cavoid_oracle as po
from tests import replay as rp

F_PRESENT, F_LEARNING = 0x20, 0x40
STRAIGHT, STOP = 2, 9                   # the default table: [1.0, 0.0] and [0.0, 0.0]
STEPS = 4                               # steps every batch is run for, and the K of the K-step launches
SEED = 71
LEARNER, STATIC, NONCOOP, ORCA = 0, 1, 2, 3

# every decision the hook names (oracle/cavoid_oracle.py::_br).  "lp": the programme closest to the preferred velocity; "dir": the
# direction-optimising programme of least penetration, over the projected lines
DECISIONS = (
    "act.off_goal", "line.apart", "line.dot1_neg", "line.cutoff", "line.left_leg", "lp.pref_outside", "lp.violated", "lp.disc_neg",
    "lp.parallel", "lp.parallel_out", "lp.den_pos", "lp.empty", "lp.clamp_lo", "lp.clamp_hi", "lp.no_point", "act.infeasible",
    "pen.deeper", "pen.parallel", "pen.same_dir", "dir.violated", "dir.disc_neg", "dir.parallel", "dir.parallel_out", "dir.den_pos",
    "dir.empty", "dir.forward", "dir.no_point", "pen.solved", "act.moving", "act.turn_clipped")

# decision -> (the sides no placement reaches with a margin, the reason).  The host test holds the list to at most three entries and
# proves that no case claims one of them
UNREACHABLE = collections.OrderedDict([
    ("dir.disc_neg", ((True,), "in exact arithmetic the projected programme of least penetration always has a point (the point it "
                               "starts from), so its line k always meets the disc; 5 million seeded worlds of 2 to 6 neighbours on "
                               "a 1/8 m grid never met the branch, nor did the 60 000 of the issue")),
    ("dir.empty", ((True,), "for the same reason an empty interval on a projected line is a product of rounding alone: the denser of "
                            "those searches met it 11 times in 2.5 million worlds, each time as a tie -- the trace did not survive "
                            "+-1e-12 on the coordinates -- so no placement takes it with a margin")),
    ("lp.pref_outside", ((True, False), "the preferred velocity is pref_speed times a unit vector: its squared length differs from "
                                        "pref_speed^2 by rounding alone, so both sides occur in every batch, never with a margin, "
                                        "and the two branches give the same velocity to an ulp")),
])
def unreachable(decision, side):
    return decision in UNREACHABLE and side in UNREACHABLE[decision][0]


# sides whose flip cannot move anything, by the structure of the code: they are claimed and traced, not flipped
FLIP_IS_A_NO_OP = {("act.infeasible", False): "the flipped branch runs _lp_least_penetration from begin = len(lines): an empty loop"}
# per branch group: the decisions no case meets at step 3 (the host test allows only those whose cases end the host's episode at step 1)
NO_STEP3 = {"default": [], "off": []}

# px py: float64; gx gy r pref speed: float32 values; pol; heading; t: time budget; act: a learner's action at every step
Agent = collections.namedtuple("Agent", "px py gx gy r pref pol heading speed t act", defaults=(50.0, STRAIGHT))
# claims: ((decision, side), ...) the host's trace holds at `step` (1-based); exact: None or (triple id, role, at_side, quantity name)
Case = collections.namedtuple("Case", "name step claims agents inexact exact", defaults=(False, None))


def A(px, py, gx, gy, r, pref, pol, heading, speed, t=50.0, act=STRAIGHT):
    return Agent(px, py, np.float32(gx), np.float32(gy), r, pref, pol, heading, speed, t, act)


def bystander(t):
    """a halted learner far from everything: it keeps the world running until its budget ends"""
    return A(-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, LEARNER, 0.0, 0.0, t, STOP)


def filler(i):
    """far static agent i: its ORCA line lies far outside every speed disc, so it never binds"""
    return A(40.0 + 2.0 * (i % 8), 40.0 + 2.0 * (i // 8), 40.0 + 2.0 * (i % 8), 40.0 + 2.0 * (i // 8), 0.125 + i * 2.0 ** -12, 1.0, STATIC, 0.0, 0.0)


# ---- hooks -----------------------------------------------------------------------------------------------------------------------------
class Trace(object):
    """records (name, decision) in order"""

    def __init__(self):
        self.seen = []

    def __call__(self, name, cond):
        cond = bool(cond)
        self.seen.append((name, cond))
        return cond

    def has(self, name, side):
        return (name, side) in self.seen


class Flip(object):
    """returns the opposite at the FIRST decision `name` that falls on `side`; everything else as it is"""

    def __init__(self, name, side):
        self.name, self.side, self.done = name, side, False

    def __call__(self, name, cond):
        cond = bool(cond)
        if not self.done and name == self.name and cond == self.side:
            self.done = True
            return not cond
        return cond


# ---- the groups ------------------------------------------------------------------------------------------------------------------------
OFF = dict(rvo_time_horizon=3.0, rvo_collab_coeff=0.7, rvo_radius_scale=1.2, rvo_max_delta_heading=math.pi / 4)
EXACT = dict(dt=0.25, near_goal_threshold=0.25, getting_close_range=0.25, collision_dist=0.0,
             rvo_time_horizon=4.0, rvo_collab_coeff=0.5, rvo_radius_scale=1.0)
GEN = dict(gen_rvo_fraction=0.0)        # generator worlds hold no ORCA agents and bring no ties of their own
Group = collections.namedtuple("Group", "name over cases")


def python_cfg(group, N):
    kw = {k: v for k, v in group.over.items() if not k.startswith("gen_")}
    return po.OracleConfig(max_agents=N, max_other_agents_observed=N - 1, **kw)


def world_of(agents, cfg):
    """the Python oracle's world of a list of Agent tuples, as world_from_arrays builds it from the pushed state"""
    n = len(agents)
    f64, f32, flags = np.zeros((4, n)), np.zeros((5, n), np.float32), np.zeros(n, np.uint32)
    for i, a in enumerate(agents):
        f64[:, i], f32[:, i], flags[i] = (a.px, a.py, a.heading, a.t), (a.gx, a.gy, a.r, a.pref, a.speed), _flags(a)
    sub = po.OracleConfig(**dict(cfg.__dict__, max_agents=n, max_other_agents_observed=max(n - 1, 1)))
    return po.World(po.world_from_arrays(f64, f32, flags, sub).agents, sub)


def _flags(a):
    return F_PRESENT | (F_LEARNING if a.pol == LEARNER else 0) | (a.pol << 8)


def host_action(agents, host, step, cfg, hook=None):
    """the host's [speed, delta heading] at `step` (1-based) of the world, through `hook`; None if the host is done before it"""
    w = world_of(agents, cfg)
    for _ in range(step - 1):
        w.step({i: a.act for i, a in enumerate(agents)})
    if w.agents[host].is_done:
        return None
    return po.rvo_action(host, w.agents, cfg, hook)


def trace_of(agents, host, step, cfg):
    t = Trace()
    act = host_action(agents, host, step, cfg, t)
    return t, act


PERTURB, PATTERNS, ACTION_TOL, FLIP_MOVES = 1e-12, 32, 1e-10, 1e-3


def perturbed(agents, rng):
    """every position coordinate and heading moved by +-PERTURB"""
    out = []
    for a in agents:
        s = rng.choice([-PERTURB, PERTURB], 3)
        out.append(a._replace(px=a.px + s[0], py=a.py + s[1], heading=a.heading + s[2]))
    return out


def conditioned(agents, host, step, cfg):
    """the trace is identical and the action moves by less than ACTION_TOL under PATTERNS sign patterns of +-PERTURB -> (ok, why)"""
    t0, a0 = trace_of(agents, host, step, cfg)
    rng = np.random.default_rng(12345)
    for k in range(PATTERNS):
        t1, a1 = trace_of(perturbed(agents, rng), host, step, cfg)
        if a1 is None or t1.seen != t0.seen:
            return False, "pattern %d: another trace" % k
        if float(np.abs(a1 - a0).max()) >= ACTION_TOL:
            return False, "pattern %d: the action moves by %g" % (k, float(np.abs(a1 - a0).max()))
    return True, ""


def flip_moves(agents, host, step, cfg, name, side):
    """|action - action with the first (name, side) decision flipped|, inf if the flipped run raises"""
    a0 = host_action(agents, host, step, cfg)
    try:
        with np.errstate(all="raise"):
            a1 = host_action(agents, host, step, cfg, Flip(name, side))
    except (ZeroDivisionError, ValueError, FloatingPointError, IndexError, OverflowError):
        return math.inf
    d = np.abs(a1 - a0)
    return math.inf if not np.isfinite(d).all() else float(d.max())


# ---- exact cases -----------------------------------------------------------------------------------------------------------------------
ONE_DT = 0.25


def _e(px, py, r, pol, speed, gx=None, gy=None, pref=1.0):
    """an agent of an exact world: heading exactly 0, a budget of one dt"""
    gx, gy = (px if pol == STATIC else px + 8.0) if gx is None else gx, py if gy is None else gy
    return A(px, py, gx, gy, r, pref, pol, 0.0, speed, ONE_DT, STRAIGHT)


def _ulps(x, k):
    """x moved by k ulps (k < 0: towards -inf)"""
    for _ in range(abs(k)):
        x = float(np.nextafter(x, math.inf if k > 0 else -math.inf))
    return x


def q_touch(agents):
    """dist_sq - comb_sq of host 0 and neighbour 1, as orca_lines computes them (radius scale 1.0)"""
    h, o = agents[0], agents[1]
    rpx, rpy = o.px - h.px, o.py - h.py
    comb = 1.0 * h.r + 1.0 * o.r
    return (rpx * rpx + rpy * rpy) - comb * comb


def _rel(agents):
    h, o = agents[0], agents[1]
    rpx, rpy = o.px - h.px, o.py - h.py
    rvx, rvy = h.speed * math.cos(h.heading) - o.speed * math.cos(o.heading), h.speed * math.sin(h.heading) - o.speed * math.sin(o.heading)
    inv_h = 1.0 / EXACT["rvo_time_horizon"]
    return rpx, rpy, rvx - inv_h * rpx, rvy - inv_h * rpy


def q_det(agents):
    rpx, rpy, wx, wy = _rel(agents)
    return rpx * wy - rpy * wx


def q_dot1(agents):
    rpx, rpy, wx, wy = _rel(agents)
    return wx * rpx + wy * rpy


def q_num(agents):
    """num of line 1 against line 0 in _lp_on_line: det2(e, p - q) of the two lines orca_lines gives the host"""
    cfg = po.OracleConfig(max_agents=len(agents), max_other_agents_observed=len(agents) - 1, **EXACT)
    lines = po.orca_lines(0, world_of(agents, cfg).agents, cfg)
    (qx, qy, ex, ey), (px, py, _, _) = lines[0], lines[1]
    return ex * (py - qy) - ey * (px - qx)


QUANTITY = {"touch": q_touch, "det": q_det, "dot1": q_dot1, "num": q_num}


FAR_LEARNER = A(-30.0, -30.0, -22.0, -30.0, 0.625, 1.0, LEARNER, 0.0, 0.0, ONE_DT, STRAIGHT)


def _touch(dy):
    """the host (r 0.5, at rest) and a static neighbour (r 0.25) on its goal axis at 0.75: dist_sq = 0.5625 = comb_sq"""
    return [_e(0.0, 0.0, 0.5, ORCA, 0.0, 4.0, 0.0), _e(_ulps(0.75, dy), 0.0, 0.25, STATIC, 0.0), FAR_LEARNER]


def _det(dy):
    """the host at full speed on heading 0 behind a static neighbour on its axis: rp = (2, 0), w = (0.5, 0), det2(rp, w) = 0; the
    neighbour moved off the axis by dy denormal ulps: the first dy whose products survive.  The static neighbour's goal is
    away from it: with the goal on its own spot its ego heading is atan2 of a denormal, which the two libraries legitimately evaluate
    differently (pi / 2 against 0 with the argument flushed) -- the case is stated without that function"""
    return [_e(0.0, 0.0, 0.25, ORCA, 1.0, 8.0, 0.0), _e(2.0, dy * 2.0 ** -1074, 0.5, STATIC, 0.0, 2.0, 8.0), FAR_LEARNER]


def _dot1(dx):
    """rp = (1, 1), the host at half speed and the neighbour at rest: w = (0.25, -0.25), dot1 = 0.  The neighbour is moved in y: in x
    dot1 has a double zero at rpx = 1 (0.25 - eps^2 / 4 rounds to 0.25 for every small eps)"""
    return [_e(0.0, 0.0, 0.25, ORCA, 0.5, 8.0, 0.0, 0.5), _e(1.0, _ulps(1.0, dx), 0.5, STATIC, 0.0), FAR_LEARNER]


def _num(dy):
    """the host (r 0.25, at rest, its goal straight below) touches a static neighbour above (r 0.5 at 0.75) and one below (r 0.125 at -0.375): both
    take the overlap branch with scale 0 -- two lines through the origin, anti-parallel: den = 0 and num = 0 (and the solved velocity
    is exactly zero: act.moving false).  The lower one nearer: its line moves up, num < 0, no point; further: it is apart, num > 0"""
    return [_e(0.0, 0.0, 0.25, ORCA, 0.0, 0.0, -4.0), _e(0.0, 0.75, 0.5, STATIC, 0.0), _e(0.0, _ulps(-0.375, dy), 0.125, STATIC, 0.0), FAR_LEARNER]


def _gt(q):
    return bool(q > 0.0)


def _lt(q):
    return bool(q < 0.0)


# triple -> (builder, quantity, the decision, the decision's predicate on the quantity: false at the threshold for all four)
TRIPLES = collections.OrderedDict([
    ("touch", (_touch, "touch", "line.apart", _gt)),         # dist_sq > comb_sq: false at equality
    ("det", (_det, "det", "line.left_leg", _gt)),            # det2(rp, w) > 0
    ("dot1", (_dot1, "dot1", "line.dot1_neg", _lt)),         # dot1 < 0
    ("num", (_num, "num", "lp.parallel_out", _lt)),          # num < 0 of coincident lines
])


def smallest_displacement(build, quantity, sign):
    """the smallest k >= 1 such that build(sign * k) moves the computed quantity off the threshold 0"""
    q = QUANTITY[quantity]
    assert q(build(0)) == 0.0
    for k in range(1, 4096):
        if q(build(sign * k)) != 0.0:
            return k
    raise AssertionError((quantity, sign, "no displacement up to 4096 ulps changes the quantity"))


def exact_cases():
    out = []
    for tid, (build, quantity, decision, pred) in TRIPLES.items():
        q = QUANTITY[quantity]
        worlds = {"at": build(0)}
        for sign in (-1, 1):
            k = smallest_displacement(build, quantity, sign)
            w = build(sign * k)
            worlds["below" if q(w) < 0.0 else "above"] = w
        assert sorted(worlds) == ["above", "at", "below"], (tid, sorted(worlds))
        for role in ("below", "at", "above"):
            side = pred(q(worlds[role]))
            out.append(Case("X-%s-%s" % (tid, role), 1, ((decision, side),), worlds[role], False, (tid, role, quantity)))
    # the branch taken and not taken where no equality is constructible: the parallel line that is skipped (two static neighbours
    # in line ahead, the farther one first) and the squeezed host whose second line has no point (mid-point line of least penetration)
    out.append(Case("X-parallel-skipped", 1, (("lp.parallel", True), ("lp.parallel_out", False)),
                    [_e(0.0, 0.0, 0.25, ORCA, 0.0, 8.0, 0.0), _e(2.5, 0.0, 0.5, STATIC, 0.0), _e(1.5, 0.0, 0.375, STATIC, 0.0), FAR_LEARNER]))
    out.append(Case("X-squeezed", 1, (("lp.parallel_out", True), ("pen.parallel", True), ("pen.same_dir", False)),
                    [_e(0.0, 0.0, 0.25, ORCA, 0.0, 0.0, -4.0), _e(0.0, 0.625, 0.5, STATIC, 0.0), _e(0.0, -0.375, 0.375, STATIC, 0.0), FAR_LEARNER]))
    return out


# ---- branch cases: the table the seeded search wrote (tools are not needed to check it: the host test proves every claim) -------------
def _case(name, step, claims, inexact, rows):
    return Case(name, step, tuple((c[:-1], c[-1] == "+") for c in claims.split()), [A(*r) for r in rows], inexact)


def on_goal():
    """equality that no margin can hold: the host stands ON its float32 goal (gn == 0: act.off_goal false, no preferred velocity) with
    nothing in its way, so the solved velocity is exactly zero (act.moving false).  Listed with the branch cases of both groups, kept out
    of their +-1e-12 test"""
    rows = [A(1.0, 0.5, 1.0, 0.5, 0.25, 1.0, ORCA, 1.0, 0.0), A(3.0, 0.5, 3.0, 0.5, 0.5, 1.0, STATIC, 0.0, 0.0), bystander(0.3)]
    return Case("on-goal", 1, (("act.off_goal", False), ("act.moving", False)), rows, False, ("on-goal", "at", None))


DEFAULT_CASES = [
    _case("D00", 1, "act.infeasible+ act.moving+ act.turn_clipped- dir.disc_neg- dir.forward- dir.no_point- dir.violated+ line.apart- line.apart+ line.cutoff+ line.dot1_neg+ lp.den_pos- lp.empty+ lp.no_point+ lp.violated+ pen.deeper+ pen.parallel- pen.solved+", True, [
        (-0.00036743110356147524, -0.0007204899324803483, -1.375, -2.75, 0.5, 1.0, 3, -2.035024306773963, 0.0, 50.0, 2),
        (2.374395735825822, -2.3746996805919607, 6.374395847320557, -2.374699592590332, 0.2509765625, 0.5, 2, -0.000956102340288334, 0.25, 50.0, 2),
        (-0.37518657250327425, 0.6252341329459751, 3.6248133182525635, 0.6252341270446777, 0.501953125, 0.5, 0, -0.0001354999560986063, 0.25, 0.30000000000000004, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("D01", 1, "act.moving+ act.off_goal+ act.turn_clipped- line.apart+ line.dot1_neg- line.left_leg- line.left_leg+ lp.clamp_hi- lp.clamp_lo- lp.disc_neg- lp.no_point- lp.violated- lp.violated+", True, [
        (-0.008157032210869018, 0.01354582592422738, 3.875, 1.75, 0.25, 1.0, 3, 0.13486002710093814, 1.0, 50.0, 2),
        (1.4091219329689444, 0.33607738571080426, 1.4091219902038574, 0.33607739210128784, 0.2509765625, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (2.257129491184862, -2.518889099034124, -1.7428704500198364, -2.5188891887664795, 0.251953125, 0.5, 0, -3.1611403764405392, 0.0, 0.30000000000000004, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("D02", 1, "act.moving+ act.turn_clipped+ line.apart- lp.clamp_hi- lp.clamp_hi+ lp.den_pos+ lp.disc_neg- lp.empty- lp.no_point- lp.parallel-", True, [
        (6.460717579859887e-07, -4.7215008067790924e-07, 2.75, -3.5, 0.5, 1.0, 3, -0.6048270383860898, 1.0, 50.0, 2),
        (0.4999996026683741, -0.25000011673121153, 0.49999961256980896, -0.25000011920928955, 0.2509765625, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (1.2500001723754897, -1.500000402031241, 1.2500001192092896, -1.5000003576278687, 0.251953125, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("D03", 1, "act.moving+ act.turn_clipped+ dir.forward+ dir.violated+ line.apart- line.cutoff+ line.dot1_neg+ lp.no_point+ lp.parallel_out+ lp.violated+ pen.same_dir-", True, [
        (-1.2692219288976728e-07, -1.3037459391895802e-07, 0.0, 2.0, 0.25, 1.0, 3, 1.5707961265493486, 0.5, 50.0, 2),
        (5.626976870193849e-07, 0.3749992569501364, 5.626976644634851e-07, -3.6250007152557373, 0.5009765625, 0.5, 0, -1.5707963752978802, 0.25, 0.30000000000000004, 2),
        (2.978253727637375e-07, -0.8749992619244327, -3.999999761581421, -0.8749992847442627, 0.251953125, 0.5, 0, -3.1415927677581856, 0.0, 0.30000000000000004, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("D04", 1, "act.moving+ act.turn_clipped- line.apart+ line.cutoff- line.cutoff+ line.dot1_neg+ line.left_leg+ lp.clamp_lo- lp.clamp_lo+ lp.den_pos- lp.disc_neg- lp.empty- lp.no_point- lp.parallel-", False, [
        (0.0, 0.0, 1.75, 2.625, 0.5, 1.0, 3, 3.982793723247329, 0.5, 50.0, 2),
        (1.375, 1.75, 1.375, 1.75, 0.2509765625, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-2.375, -0.375, -2.375, -0.375, 0.501953125, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("D05", 1, "act.moving+ act.turn_clipped+ line.apart- lp.disc_neg+ lp.no_point+ pen.parallel+ pen.same_dir+", False, [
        (0.0, 0.0, 6.0, 0.0, 0.5, 1.0, 3, 3.0, 0.0, 50.0, 2),
        (-2.375, 0.0, -2.375, 0.0, 0.2509765625, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-0.125, 0.0, -0.125, 0.0, 0.251953125, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("D06", 1, "act.moving+ act.turn_clipped- line.apart- lp.disc_neg- lp.no_point- lp.parallel+ lp.parallel_out-", False, [
        (0.0, 0.0, 0.0, -2.0, 0.5, 1.0, 3, 1.4292036732051034, 0.0, 50.0, 2),
        (0.0, -1.375, 2.8284270763397217, -4.203427314758301, 0.2509765625, 0.5, 0, -0.7853981633974483, 0.0, 0.30000000000000004, 2),
        (0.0, -0.75, 0.0, -0.75, 0.251953125, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("D07", 1, "act.infeasible+ act.moving+ act.turn_clipped+ dir.violated- line.apart- lp.disc_neg+ lp.no_point+ pen.deeper+ pen.solved+", False, [
        (0.0, 0.0, -2.75, 3.75, 0.25, 0.5, 3, 5.20354516179708, 0.5, 50.0, 2),
        (-1.25, 0.0, -4.078427314758301, 2.8284270763397217, 0.2509765625, 0.5, 0, 2.356194490192345, 0.25, 0.30000000000000004, 2),
        (0.25, 0.0, 3.0784270763397217, 2.8284270763397217, 0.501953125, 1.0, 0, 0.7853981633974483, 1.0, 0.30000000000000004, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("D08", 1, "act.infeasible+ act.moving+ act.turn_clipped- line.apart- lp.disc_neg+ lp.no_point+ lp.violated+ pen.deeper- pen.deeper+ pen.solved+", True, [
        (0.0008184399111610295, -0.0008570057365813679, 0.0, -2.0, 0.5, 1.0, 3, -1.8699213741788785, 1.0, 50.0, 2),
        (0.0008797309261923889, -0.1259395003302064, 0.0008797309128567576, -0.1259395033121109, 0.5009765625, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-0.0009280603271804837, -0.24954870501032383, -0.0009280603262595832, 3.7504513263702393, 0.501953125, 1.0, 2, 1.5713517373586336, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("D09", 1, "act.moving+ act.turn_clipped- dir.no_point+ dir.parallel+ dir.parallel_out+ line.apart- line.cutoff+ lp.disc_neg+ lp.no_point+ pen.same_dir- pen.solved-", True, [
        (-4.023063985218269e-07, -9.848679271440232e-07, 0.0, 4.0, 0.5, 1.0, 3, 1.8707954868467596, 0.0, 50.0, 2),
        (-2.1218736952487168e-07, -0.9999999649544681, -4.0, -0.9999999403953552, 0.2509765625, 0.5, 3, -3.1415932206854666, 0.25, 50.0, 2),
        (-2.3962560772673175e-07, -1.7500003611647776, -2.3962562067936233e-07, 2.249999523162842, 0.251953125, 1.0, 2, 1.5707956955226414, 0.0, 50.0, 2),
        (9.747369827276348e-07, -0.12500013876657123, 9.74736963144096e-07, -0.12500013411045074, 0.2529296875, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (4.442539702969359e-07, 0.500000541941609, 2.82842755317688, 3.32842755317688, 0.50390625, 0.5, 3, 0.7853979922167388, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("D10", 1, "act.infeasible+ act.moving+ act.turn_clipped- dir.disc_neg- dir.empty- dir.forward- dir.forward+ dir.no_point- dir.parallel_out- dir.violated- dir.violated+ line.apart- line.apart+ line.cutoff+ line.dot1_neg+ lp.disc_neg+ lp.no_point+ pen.deeper- pen.deeper+ pen.parallel- pen.same_dir- pen.same_dir+ pen.solved+", True, [
        (4.833371260779392e-10, -9.462719512483797e-07, 0.0, -4.0, 0.25, 0.5, 3, -0.570796840273481, 0.0, 50.0, 2),
        (4.114911099068782e-07, -2.2499999676032054, 4.114911007491173e-07, 1.75, 0.2509765625, 0.5, 3, 1.5707956328228811, 0.25, 50.0, 2),
        (8.980769278474198e-07, 2.1250005413956594, 8.980769052868709e-07, 2.125000476837158, 0.501953125, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (-9.013511285291331e-07, 0.12499974120195288, -9.013511430566723e-07, 4.124999523162842, 0.2529296875, 1.0, 2, 1.5707962005022242, 1.0, 50.0, 2),
        (-9.705982275417122e-07, 1.1250002808764894, -9.705981938168406e-07, 5.125000476837158, 0.50390625, 0.5, 3, 1.570795340098264, 0.5, 50.0, 2),
        (0.7499992891659725, -4.176213966064877e-07, 0.7499992847442627, -4.176214076778706e-07, 0.2548828125, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("D11", 1, "act.infeasible+ act.moving+ act.turn_clipped- dir.den_pos- dir.den_pos+ dir.disc_neg- dir.empty- dir.no_point- dir.parallel- dir.parallel_out- line.apart- line.cutoff+ line.dot1_neg+ lp.disc_neg+ lp.no_point+ pen.deeper+ pen.solved+", True, [
        (-9.86373208532253e-07, 1.9501098045869275e-07, -2.0, 0.0, 0.25, 1.0, 3, 4.141592189991664, 0.0, 50.0, 2),
        (-2.5000007215096764, 4.763118429123436e-07, -6.500000953674316, 4.7631183974772284e-07, 0.5009765625, 1.0, 3, -3.1415916667495023, 1.0, 50.0, 2),
        (-2.125000064089729, -7.287194101719691e-07, 1.8749998807907104, -7.287193852789642e-07, 0.251953125, 0.5, 0, -9.822333589350543e-07, 0.25, 0.30000000000000004, 2),
        (-0.500000059136924, 1.501639134423474e-08, -3.3284270763397217, -2.8284270763397217, 0.2529296875, 0.5, 2, -2.356194124654959, 0.5, 50.0, 2),
        (-0.749999221911482, -8.794400851032249e-07, -0.7499992251396179, -8.794401082923287e-07, 0.50390625, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (0.37500045761043155, 9.899770352876607e-07, -3.624999523162842, 9.899770248011919e-07, 0.5048828125, 1.0, 0, -3.141593638794571, 0.5, 0.30000000000000004, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("D12", 3, "act.off_goal+ act.turn_clipped- lp.clamp_hi- lp.clamp_lo- lp.disc_neg- lp.no_point- lp.parallel+ lp.parallel_out- lp.violated- lp.violated+", False, [
        (0.0, 0.0, 6.0, 0.0, 0.5, 0.5, 3, 0.0, 0.0, 50.0, 2),
        (-1.125, 0.0, -1.125, 0.0, 0.2509765625, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (2.0, 0.0, 2.0, 0.0, 0.251953125, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.7000000000000001, 9),
    ]),
    _case("D13", 3, "act.infeasible+ act.moving+ act.turn_clipped+ dir.disc_neg- dir.forward- dir.no_point- dir.violated+ line.apart- line.apart+ line.cutoff+ line.dot1_neg+ lp.no_point+ lp.parallel_out+ lp.violated+ pen.deeper+ pen.same_dir- pen.solved+", True, [
        (-7.69826407823162e-07, -6.966796518372056e-07, 2.0, 0.0, 0.5, 1.0, 3, 1.5707953277344517, 0.0, 50.0, 2),
        (1.2500009161955645, 1.225125851545271e-07, -2.7499990463256836, 1.2251258851847524e-07, 0.5009765625, 0.5, 0, -3.1415926492863595, 0.5, 0.7000000000000001, 2),
        (-1.7500006979117944, 8.978272784753021e-07, -1.7500007152557373, 8.978273058346531e-07, 0.501953125, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.7000000000000001, 9),
    ]),
    _case("D14", 3, "act.infeasible+ act.moving+ act.turn_clipped- dir.disc_neg- dir.forward+ dir.no_point- dir.violated+ line.apart+ line.cutoff+ line.dot1_neg- line.dot1_neg+ line.left_leg- lp.den_pos+ lp.empty+ lp.no_point+ lp.violated+ pen.deeper+ pen.parallel- pen.solved+", False, [
        (0.0, 0.0, 3.5, 1.75, 0.5, 0.5, 3, 0.4636476090008061, 0.25, 50.0, 2),
        (2.375, 1.0, 2.375, 1.0, 0.5009765625, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-1.375, -0.125, 2.625, -0.125, 0.251953125, 1.0, 0, 0.0, 1.0, 0.7000000000000001, 2),
        (-1.0, -2.375, 1.8284270763397217, -5.203427314758301, 0.2529296875, 1.0, 2, -0.7853981633974483, 1.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.7000000000000001, 9),
    ]),
    _case("D15", 3, "act.infeasible+ act.moving+ act.turn_clipped+ dir.den_pos- dir.disc_neg- dir.empty- dir.forward+ dir.no_point- dir.parallel- line.left_leg+ lp.no_point+ pen.deeper+ pen.solved+", False, [
        (0.0, 0.0, 2.5, 3.25, 0.5, 1.0, 3, 3.9151007005533605, 0.0, 50.0, 2),
        (2.0, -0.75, -2.0, -0.75, 0.2509765625, 0.5, 3, -3.141592653589793, 0.5, 50.0, 2),
        (1.375, 0.875, 1.375, 0.875, 0.251953125, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-1.875, 0.375, 2.125, 0.375, 0.5029296875, 1.0, 0, 0.0, 0.5, 0.7000000000000001, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.7000000000000001, 9),
    ]),
    _case("D16", 3, "act.infeasible+ act.moving+ act.turn_clipped- dir.den_pos- dir.disc_neg- dir.empty- dir.no_point- dir.parallel_out- dir.violated- line.dot1_neg- line.left_leg+ lp.no_point+ pen.deeper+ pen.parallel- pen.solved+", True, [
        (-8.033855345463598e-07, 2.6169500752584627e-07, 0.0, 2.0, 0.5, 0.5, 3, 1.870796889263481, 0.0, 50.0, 2),
        (6.836403212640053e-07, -1.375000977912206, 6.836403372290079e-07, -1.3750009536743164, 0.5009765625, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (5.057802719322218e-07, 2.1249998930403455, 5.057802923147392e-07, 2.125, 0.501953125, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-4.146526361532427e-07, -1.3749992703413667, -4.1465264644102717e-07, -1.3749992847442627, 0.5029296875, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (-1.9630449008405162e-07, 0.9999993505442956, -1.9630448377938592e-07, -3.0000007152557373, 0.25390625, 0.5, 2, -1.5707966303643024, 0.5, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.7000000000000001, 9),
    ]),
]
OFF_CASES = [
    _case("O00", 1, "act.infeasible+ act.moving+ act.turn_clipped- dir.disc_neg- dir.forward+ dir.no_point- dir.violated+ line.apart- line.apart+ line.cutoff- line.left_leg+ lp.den_pos+ lp.empty+ lp.no_point+ lp.violated+ pen.deeper+ pen.parallel- pen.solved+", True, [
        (3.6957244268586567e-07, 1.5711330319588127e-07, -2.0, -0.125, 0.25, 0.5, 3, -2.0791733417963756, 0.5, 50.0, 2),
        (-1.1249993094557014, -0.4999997504192169, -1.1249992847442627, -4.499999523162842, 0.2509765625, 1.0, 3, -1.5707956005326078, 0.0, 50.0, 2),
        (0.6249996124342843, -0.37499915487918545, 4.624999523162842, -0.37499916553497314, 0.501953125, 1.0, 2, 3.7352457391080435e-07, 0.5, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("O01", 1, "act.moving+ act.off_goal+ act.turn_clipped- line.dot1_neg- line.left_leg+ lp.clamp_hi- lp.clamp_lo- lp.den_pos- lp.disc_neg- lp.empty- lp.no_point- lp.violated- lp.violated+", True, [
        (-8.380775963212246e-07, -7.564172159632052e-08, 0.0, 2.0, 0.5, 1.0, 3, 1.5707972806856219, 1.0, 50.0, 2),
        (-6.70799805978792e-07, -1.5000007596326477, 2.8284263610839844, -4.328427791595459, 0.5009765625, 0.5, 0, -0.7853978322510964, 0.25, 0.30000000000000004, 2),
        (6.229642946350546e-07, 1.2499992400495636, 6.229643076949287e-07, 1.2499992847442627, 0.501953125, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("O02", 1, "act.infeasible+ act.moving+ act.turn_clipped+ dir.disc_neg- dir.forward- dir.no_point- dir.violated+ line.apart- line.apart+ line.cutoff+ line.dot1_neg+ lp.no_point+ lp.parallel_out+ lp.violated+ pen.deeper+ pen.same_dir- pen.solved+", True, [
        (-3.981182246043398e-07, 2.636815826340584e-09, 4.0, 0.0, 0.25, 1.0, 3, -6.199925594161415e-07, 0.5, 50.0, 2),
        (1.7500005200171715, -4.523312240345609e-07, 1.7500004768371582, -4.523312213677855e-07, 0.2509765625, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-0.874999511648186, -8.293749427015512e-07, 3.125000476837158, -8.293749260701588e-07, 0.501953125, 0.5, 3, 2.334858832097799e-07, 0.25, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("O03", 1, "act.moving+ act.turn_clipped+ line.apart- lp.disc_neg+ lp.no_point+ pen.parallel+ pen.same_dir+", False, [
        (0.0, 0.0, 6.0, 0.0, 0.5, 1.0, 3, 3.0, 0.0, 50.0, 2),
        (-2.375, 0.0, -2.375, 0.0, 0.2509765625, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-0.125, 0.0, -0.125, 0.0, 0.251953125, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("O04", 1, "act.moving+ act.turn_clipped+ line.apart- line.cutoff+ lp.clamp_hi- lp.clamp_hi+ lp.den_pos+ lp.disc_neg- lp.empty- lp.no_point- lp.parallel-", True, [
        (-0.0009603861778981456, -0.0008058727496565972, 2.25, 2.25, 0.5, 1.0, 3, 1.0859180577054142, 0.0, 50.0, 2),
        (0.12501067959937862, 0.8752241191891292, 0.125010684132576, 0.8752241134643555, 0.2509765625, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (1.3758548974677034, -2.49906134742177, 1.3758548498153687, 1.5009386539459229, 0.501953125, 1.0, 2, 1.5699384521490296, 1.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("O05", 1, "act.moving+ act.turn_clipped- line.apart- lp.disc_neg- lp.no_point- lp.parallel+ lp.parallel_out-", False, [
        (0.0, 0.0, 0.0, -2.0, 0.5, 1.0, 3, 1.4292036732051034, 0.0, 50.0, 2),
        (0.0, -1.375, 2.8284270763397217, -4.203427314758301, 0.2509765625, 0.5, 0, -0.7853981633974483, 0.0, 0.30000000000000004, 2),
        (0.0, -0.75, 0.0, -0.75, 0.251953125, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("O06", 1, "act.moving+ act.off_goal+ act.turn_clipped- line.apart+ line.left_leg- line.left_leg+ lp.clamp_lo+ lp.disc_neg- lp.no_point- lp.violated- lp.violated+", True, [
        (4.82194785731895e-07, -9.553932880176805e-08, 2.0, -1.25, 0.25, 1.0, 3, -0.8586002074738811, 1.0, 50.0, 2),
        (1.9999991511611597, -0.12499946050131311, 1.9999991655349731, -0.12499946355819702, 0.5009765625, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (1.1250008440150112, -2.0000002681575673, 1.1250008344650269, -2.000000238418579, 0.251953125, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("O07", 1, "act.infeasible+ act.moving+ act.turn_clipped+ dir.violated- line.apart- lp.disc_neg+ lp.no_point+ lp.violated+ pen.deeper+ pen.solved+", False, [
        (0.0, 0.0, -4.0, 0.0, 0.25, 0.5, 3, 2.8415926535897933, 0.5, 50.0, 2),
        (-2.375, 0.0, -2.375, 4.0, 0.2509765625, 1.0, 0, 1.5707963267948966, 1.0, 0.30000000000000004, 2),
        (-0.25, 0.0, 3.75, 0.0, 0.251953125, 0.5, 3, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("O08", 1, "act.infeasible+ act.moving+ act.turn_clipped- line.apart- lp.disc_neg+ lp.no_point+ lp.violated+ pen.deeper- pen.deeper+ pen.solved+", True, [
        (0.0008184399111610295, -0.0008570057365813679, 0.0, -2.0, 0.5, 1.0, 3, -1.8699213741788785, 1.0, 50.0, 2),
        (0.0008797309261923889, -0.1259395003302064, 0.0008797309128567576, -0.1259395033121109, 0.5009765625, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-0.0009280603271804837, -0.24954870501032383, -0.0009280603262595832, 3.7504513263702393, 0.501953125, 1.0, 2, 1.5713517373586336, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("O09", 1, "act.moving+ act.turn_clipped- dir.no_point+ dir.parallel+ dir.parallel_out+ dir.violated+ line.apart- line.cutoff+ lp.disc_neg+ lp.no_point+ pen.same_dir- pen.solved-", True, [
        (-4.023063985218269e-07, -9.848679271440232e-07, 0.0, 4.0, 0.5, 1.0, 3, 1.8707954868467596, 0.0, 50.0, 2),
        (-2.1218736952487168e-07, -0.9999999649544681, -4.0, -0.9999999403953552, 0.2509765625, 0.5, 3, -3.1415932206854666, 0.25, 50.0, 2),
        (-2.3962560772673175e-07, -1.7500003611647776, -2.3962562067936233e-07, 2.249999523162842, 0.251953125, 1.0, 2, 1.5707956955226414, 0.0, 50.0, 2),
        (9.747369827276348e-07, -0.12500013876657123, 9.74736963144096e-07, -0.12500013411045074, 0.2529296875, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (4.442539702969359e-07, 0.500000541941609, 2.82842755317688, 3.32842755317688, 0.50390625, 0.5, 3, 0.7853979922167388, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("O10", 1, "act.infeasible+ act.moving+ act.turn_clipped- dir.den_pos- dir.disc_neg- dir.empty- dir.no_point- dir.parallel_out- dir.violated- line.apart- line.left_leg- lp.disc_neg+ lp.no_point+ pen.deeper+ pen.solved+", True, [
        (-6.432655517241879e-08, 5.748152197812935e-07, 0.0, 2.0, 0.25, 0.5, 3, 4.570795416047605, 0.0, 50.0, 2),
        (-9.351634561300561e-07, -1.8749998981524327, 3.9999990463256836, -1.8749998807907104, 0.2509765625, 1.0, 0, 1.4543895566706182e-07, 1.0, 0.30000000000000004, 2),
        (-8.96516267765159e-08, 0.8750003996317209, -8.965162834329021e-08, 0.8750004172325134, 0.251953125, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-6.203319589681723e-07, -1.5000003569097968, 2.8284265995025635, 1.328426718711853, 0.2529296875, 1.0, 2, 0.7853973237675567, 1.0, 50.0, 2),
        (-6.311585603885817e-07, 0.750000054854669, -6.311585707408085e-07, 0.7500000596046448, 0.50390625, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-8.212977536250854e-07, -1.5000006262900256, 3.9999992847442627, -1.5000005960464478, 0.5048828125, 1.0, 0, 6.443356275731197e-07, 0.5, 0.30000000000000004, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("O11", 1, "act.moving+ act.turn_clipped+ dir.den_pos+ dir.empty- dir.forward- dir.parallel- line.apart- line.cutoff+ lp.no_point+ lp.violated+ pen.deeper-", False, [
        (0.0, 0.0, 2.375, -1.75, 0.25, 1.0, 3, -0.9350267353903137, 0.0, 50.0, 2),
        (0.625, -0.25, -2.2034270763397217, -3.0784270763397217, 0.5009765625, 1.0, 2, -2.356194490192345, 1.0, 50.0, 2),
        (-1.875, -2.0, -1.875, 2.0, 0.501953125, 1.0, 2, 1.5707963267948966, 1.0, 50.0, 2),
        (-1.25, 1.25, -1.25, 1.25, 0.5029296875, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-0.125, -0.875, 2.7034270763397217, -3.7034270763397217, 0.25390625, 0.5, 3, -0.7853981633974483, 0.0, 50.0, 2),
        (-0.625, 2.125, -0.625, 2.125, 0.2548828125, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.30000000000000004, 9),
    ]),
    _case("O12", 3, "act.infeasible+ act.moving+ act.turn_clipped+ dir.disc_neg- dir.forward- dir.no_point- dir.violated+ line.apart- line.apart+ lp.no_point+ lp.parallel_out+ lp.violated+ pen.deeper+ pen.same_dir- pen.solved+", True, [
        (-6.357373503445611e-07, -8.16750541533833e-08, 2.0, 0.0, 0.5, 1.0, 3, 3.0000001765703823, 0.5, 50.0, 2),
        (2.000000185008131, 8.556892233481959e-07, 2.000000238418579, 8.556892225897172e-07, 0.2509765625, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (-1.1250008508946803, -3.084413140300825e-07, -1.1250008344650269, -3.0844131515550544e-07, 0.501953125, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.7000000000000001, 9),
    ]),
    _case("O13", 3, "act.moving+ act.off_goal+ act.turn_clipped- line.apart+ lp.clamp_hi+ lp.clamp_lo- lp.den_pos+ lp.disc_neg- lp.empty- lp.no_point- lp.parallel- lp.violated+", False, [
        (0.0, 0.0, -0.875, 0.625, 0.25, 1.0, 3, 1.5213431676069717, 0.0, 50.0, 2),
        (-1.625, -0.75, 2.375, -0.75, 0.2509765625, 0.5, 2, 0.0, 0.0, 50.0, 2),
        (-0.625, 0.75, -0.625, 0.75, 0.501953125, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (0.875, 2.375, 0.875, 2.375, 0.2529296875, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.7000000000000001, 9),
    ]),
    _case("O14", 3, "act.infeasible+ act.moving+ act.turn_clipped- dir.disc_neg- dir.no_point- dir.parallel_out- line.apart- lp.no_point+ lp.parallel_out+ pen.deeper+ pen.solved+", False, [
        (0.0, 0.0, 0.0, -4.0, 0.5, 0.5, 3, 0.0, 0.5, 50.0, 2),
        (0.0, -1.75, 0.0, -1.75, 0.5009765625, 1.0, 1, 0.0, 0.0, 50.0, 2),
        (0.0, -1.125, 2.4492937051703357e-16, 2.875, 0.501953125, 0.5, 3, 1.5707963267948966, 0.0, 50.0, 2),
        (0.0, 2.125, 0.0, 2.125, 0.2529296875, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.7000000000000001, 9),
    ]),
    _case("O15", 3, "act.infeasible+ act.moving+ act.turn_clipped- dir.den_pos- dir.disc_neg- dir.empty- dir.forward- dir.forward+ dir.no_point- dir.parallel- dir.violated- dir.violated+ line.apart- line.apart+ line.cutoff- line.cutoff+ line.dot1_neg+ line.left_leg+ lp.disc_neg+ lp.no_point+ pen.deeper+ pen.parallel- pen.solved+", True, [
        (0.03396611024987955, 0.03741679060765326, 2.875, -4.0, 0.5, 0.5, 3, -0.6698633478376081, 0.0, 50.0, 2),
        (-1.784891330883042, -0.28228894448953024, -1.7848913669586182, -0.28228893876075745, 0.5009765625, 0.5, 1, 0.0, 0.0, 50.0, 2),
        (2.4942241256490885, -1.3749701477987286, -1.5057759284973145, -1.3749701976776123, 0.501953125, 1.0, 3, -3.117994919096416, 0.5, 50.0, 2),
        (-1.7772848879391172, -0.724465086840894, -5.777285099029541, -0.7244650721549988, 0.2529296875, 1.0, 0, -3.1704584971838146, 0.5, 0.7000000000000001, 2),
        (1.02153547256376, 0.22989105253002054, -2.9784646034240723, 0.22989104688167572, 0.25390625, 0.5, 2, -3.1024332486906943, 0.25, 50.0, 2),
        (-1.121487477598136, 1.1271471632693546, 1.706939697265625, 3.9555742740631104, 0.2548828125, 0.5, 2, 0.7794817703325663, 0.0, 50.0, 2),
        (-30.0, -30.0, -20.0, -30.0, 0.375, 1.0, 0, 0.0, 0.0, 0.7000000000000001, 9),
    ]),
]
DEFAULT_CASES.append(on_goal())
OFF_CASES.append(on_goal())


def _groups():
    g = [Group("default", dict(GEN), DEFAULT_CASES), Group("off", dict(GEN, **OFF), OFF_CASES), Group("exact", dict(GEN, **EXACT), exact_cases())]
    return collections.OrderedDict((x.name, x) for x in g)


GROUPS = _groups()


def over_of(group, rvo_enabled=None):
    return dict(group.over) if rvo_enabled is None else dict(group.over, rvo_enabled=rvo_enabled)


# ---- layout ----------------------------------------------------------------------------------------------------------------------------
Placed = collections.namedtuple("Placed", "case variant host agents")       # agents: the N rows of the world (None: absent)


def layouts(case, c, N):
    """the three placements of case number c at N agents per world"""
    host, others = case.agents[0], list(case.agents[1:])
    room = N - len(case.agents)
    fill = [filler(i) for i in range(room)]
    absent = [None] * room
    first = absent if c % 4 == 3 else fill
    return [Placed(case, 0, 0, [host] + others + first),
            Placed(case, 1, len(others), others + [host] + fill),
            Placed(case, 2, N - 1, fill + others + [host])]


def cases_of(group, N):
    return [c for c in group.cases if len(c.agents) <= N]


def world_index(c, v):
    return 6 * c + (c + v) % 3


def num_worlds(group, N):
    return 6 * len(cases_of(group, N))


def placed_worlds(group, N):
    """[(world index, Placed)]"""
    out = []
    for c, case in enumerate(cases_of(group, N)):
        for p in layouts(case, c, N):
            out.append((world_index(c, p.variant), p))
    return out


def oracle_for(group, N):
    return rp.oracle_for(N, N - 1, **group.over)


def place(group, N, st):
    for w, p in placed_worlds(group, N):
        base = w * N
        sl = slice(base, base + N)
        st.f64[:, sl], st.f32[:, sl], st.flags[sl] = 0.0, 0.0, 0
        for i, a in enumerate(p.agents):
            if a is None:
                continue
            st.f64[:, base + i] = (a.px, a.py, a.heading, a.t)
            st.f32[:, base + i] = (a.gx, a.gy, a.r, a.pref, a.speed)
            st.flags[base + i] = _flags(a)
            assert float(np.float32(a.r)) == a.r and float(np.float32(a.pref)) == a.pref and float(np.float32(a.speed)) == a.speed, p.case.name


def actions(group, N, W):
    acts = np.full((STEPS, W, N), STRAIGHT, np.int32)
    for w, p in placed_worlds(group, N):
        for i, a in enumerate(p.agents):
            if a is not None:
                acts[:, w, i] = a.act
    return acts


class Run(object):
    """the C oracle over one group at N agents: generator worlds from the reset, the placed ones written over them, the observation of
    the pushed state, ONE plain step from it (what env.step is held to) and STEPS auto-reset steps -- computed once, shared by the tests
    of a session and never changed"""
    _cache = {}

    def __init__(self, group, N):
        self.group, self.N, self.W = group, N, num_worlds(group, N)
        self.cfg, self.gen = oracle_for(group, N)
        st = co.State.empty(self.W, N)
        self.ep = np.zeros(self.W, np.uint32)
        co.generate(self.cfg, self.gen, SEED, st, self.ep)
        place(group, N, st)
        self.start = st.copy()
        self.acts = actions(group, N, self.W)
        self.obs0 = co.observe(self.cfg, st)
        plain = st.copy()
        self.plain_out = co.step(self.cfg, plain, self.acts[0])
        self.plain_state = plain
        self.outs, self.states, self.eps = [], [], []
        for t in range(STEPS):
            self.outs.append(co.step_autoreset(self.cfg, self.gen, SEED, st, self.ep, self.acts[t]))
            self.states.append(st.copy())
            self.eps.append(self.ep.copy())

    @classmethod
    def of(cls, name, N):
        key = (name, N)
        if key not in cls._cache:
            cls._cache[key] = cls(GROUPS[name], N)
        return cls._cache[key]

    def placed(self):
        return placed_worlds(self.group, self.N)
