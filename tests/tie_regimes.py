"""Shared cases of the tests that hold the env step to the oracle AT its comparisons: exact ties of the sort keys and exact equality in
the threshold predicates (the pattern of tests/cfg_regimes.py and tests/policy_regimes.py).  A plain module: tests/test_tie_regimes_host.py
(CPU: both oracles, the straddles, the ties) and tests/test_gpu_tie_regimes.py (every launch form) build the SAME batches from it.

Generator scenarios and uniform random states never put a float64 gap ON collision_dist or two neighbours on one 63-bit sort key, so the
worlds here are placed by hand and pushed with set_state.  They are made of exactly representable numbers -- dt = 0.25; thresholds of
0.25; radii, speeds and positions that are small multiples of powers of two; movers on heading exactly 0 taking the straight-ahead
action (0.25 m per step, added without rounding) -- so that equality is real.  Every threshold is a TRIPLE of worlds: one ulp below, at,
one ulp above (or, where an ulp cannot change the branch, the branch taken and not taken), reached after k = 1 and after k = 4 moves, so
that a K-step launch meets it at two different steps inside the launch.  The hand-placed worlds sit at every third world of the batch;
generator worlds fill the rest and share their tiles.

Groups: one cavoid_cfg each (a threshold or a switch is a field of the configuration, so the cases that need another value run in
another env).  Worlds: the first agents of the world are placed, the rest absent; `line` worlds have all N agents present."""
import collections
import math

import numpy as np

from oracle import c_oracle as co
from oracle.cavoid_oracle import build_action_table
from tests import replay as rp

F_AT_GOAL, F_RAN_OUT, F_IN_COLL, F_PRESENT, F_LEARNING = 1, 2, 4, 0x20, 0x40
STRAIGHT, HALF, STOP = 2, 6, 9          # the default table: [1.0, 0.0], [0.5, 0.0], [0.0, 0.0] (-pi/6 + 2 * pi/12 is an exact 0.0)
TURN_PI, TURN_MPI, TURN_PI_LO, TURN_MPI_LO, TURN_PI_HI, TURN_MPI_HI = 0, 1, 3, 4, 5, 7      # PI_TABLE's rows
STEPS = 8                               # steps every case is run for: the 8-slot relay ring once, the 4-slot ring twice
SEED = 53
STRIDE = 3                              # hand-placed world k sits at world 3 k + 1
ULP_UP, ULP_DOWN = math.inf, -math.inf
PI_LO, PI_HI = np.nextafter(np.pi, 0.0), np.nextafter(np.pi, 4.0)

BASE = dict(dt=0.25, near_goal_threshold=0.25, getting_close_range=0.25, collision_dist=0.0)


def _pi_table():
    t = build_action_table()
    t[TURN_PI], t[TURN_MPI] = (1.0, np.pi), (1.0, -np.pi)
    t[TURN_PI_LO], t[TURN_MPI_LO] = (1.0, PI_LO), (1.0, -PI_LO)
    t[TURN_PI_HI], t[TURN_MPI_HI] = (1.0, PI_HI), (1.0, -PI_HI)
    assert tuple(t[STRAIGHT]) == (1.0, 0.0) and tuple(t[STOP]) == (0.0, 0.0) and tuple(t[HALF]) == (0.5, 0.0)
    return t


PI_TABLE = _pi_table()

# pol: 0 learner, 1 static.  act: one table index, or one per step.  The goal is float32 (the state holds it so), everything else float64
Agent = collections.namedtuple("Agent", "px py gx gy r pref pol heading t act", defaults=(1.0, 0, 0.0, 50.0, STRAIGHT))
# probe: (triple id, role in below / at / above, the role 'at' must equal (or None), step index, host, what is read)
Probe = collections.namedtuple("Probe", "triple role at_side step host read")
# tie: host, the tied neighbours (agent indices), the step indices (-1: the pushed state) at which they share a fast key, kind in
#   full (bucket and float64 lateral equal) / f32 (float64 laterals differ) / gap32 (exact-gap keys: float32 gaps equal) / index (bucket)
Tie = collections.namedtuple("Tie", "host group steps kind")
World = collections.namedtuple("World", "name agents probe tie order", defaults=(None, None, None))


def static(px, py, r, goal_away=False):
    """a static agent (policy 1).  Its goal is its own spot: it is AT its goal, and done, from the first step on -- under U4 flipped a done
    agent is out of the collision test, so the cases of those groups put the goal away (goal_away)"""
    return Agent(px, py, np.float32(50.0) if goal_away else np.float32(px), np.float32(py), r, 1.0, 1, 0.0, 50.0, STOP)


def mover(px, py, r, pref=1.0, gx=50.0, t=50.0, act=STRAIGHT):
    return Agent(px, py, gx, py, r, pref, 0, 0.0, t, act)


def halted(px, py, r, gx=50.0, gy=None, t=50.0):
    """a learner that takes the zero-speed action: it stays where it is and keeps its world running"""
    gy = py if gy is None else gy
    return Agent(px, py, gx, gy, r, 1.0, 0, math.atan2(gy - py, gx - px), t, STOP)


BYSTANDER = halted(0.0, 24.0, 0.75)     # keeps the world running behind the host's last step, so that the host's flags stay in the state
ROLES = (("below", ULP_DOWN), ("at", None), ("above", ULP_UP))


def _ulp(x, towards):
    return x if towards is None else float(np.nextafter(x, towards))


def _arrivals():
    return (1, 4)


# ---- threshold predicates ------------------------------------------------------------------------------------------------------------
def p1_collision(cd, goal_away=False):
    """P1  gap <= collision_dist.  Mover (r 0.5) from x0 arrives at x = 0.25 after k moves; a static agent (r 0.5) at 1.25 + cd: centre
    distance 1.0 + cd, gap cd exactly.  One ulp nearer it is hit as well, one ulp further it is not (and is not hit a step earlier: the gap
    was 0.25 larger)."""
    out = []
    for k in _arrivals():
        for role, to in ROLES:
            out.append(World("P1-cd%g-k%d-%s" % (cd, k, role), [mover(0.25 - 0.25 * k, 0.0, 0.5), static(_ulp(1.25 + cd, to), 0.0, 0.5, goal_away), BYSTANDER],
                             Probe("P1-cd%g-k%d" % (cd, k), role, "below", k - 1, 0, ("flag", F_IN_COLL, "rew"))))
    return out


def p2_close(goal_away=False):
    """P2  min_gap <= getting_close_range (0.25): the static agent at 1.5.  At equality the reward is r_close + slope * 0.25 = -0.1 +
    0.125 (the oracle's numbers, asserted in the host test); one ulp further it is reward_time_step = 0."""
    out = []
    for k in _arrivals():
        for role, to in ROLES:
            out.append(World("P2-k%d-%s" % (k, role), [mover(0.25 - 0.25 * k, 0.0, 0.5), static(_ulp(1.5, to), 0.0, 0.5, goal_away), BYSTANDER],
                             Probe("P2-k%d" % k, role, "below", k - 1, 0, ("rew",))))
    return out


def p3_horizon(h=1.25):
    """P3  d > sensing_horizon (1.25).  One neighbour at the horizon (count 1 <-> 0, slot zeroed), and two neighbours of which the far one
    is at the horizon (count 2 <-> 1: under closest_last the near one moves from slot 1 to slot 0)."""
    out = []
    for k in _arrivals():
        x0 = 0.25 - 0.25 * k
        for role, to in ROLES:
            out.append(World("P3-one-k%d-%s" % (k, role), [mover(x0, 0.0, 0.25), static(_ulp(0.25 + h, to), 0.0, 0.25)],
                             Probe("P3-one-k%d" % k, role, "below", k - 1, 0, ("nobs", "slots"))))
            out.append(World("P3-two-k%d-%s" % (k, role), [mover(x0, 0.0, 0.25), static(_ulp(0.25 + h, to), 0.0, 0.25), static(0.25, -0.75, 0.125)],
                             Probe("P3-two-k%d" % k, role, "below", k - 1, 0, ("nobs", "slots"))))
    return out


def p4_goal():
    """P4  d^2 <= near_goal^2.  The float32 goal at 0.5, the mover arrives at 0.25: d^2 = 0.0625 = thr^2 exactly.  One float32 ulp."""
    out = []
    for k in _arrivals():
        for role, to in ROLES:
            gx = np.float32(0.5) if to is None else np.nextafter(np.float32(0.5), np.float32(to))
            out.append(World("P4-k%d-%s" % (k, role), [mover(0.25 - 0.25 * k, 0.0, 0.25, gx=gx), BYSTANDER],
                             Probe("P4-k%d" % k, role, "below", k - 1, 0, ("flag", F_AT_GOAL, "rew"))))
    return out


def p5_timeout():
    """P5  t_remaining <= 0 after k steps of 0.25 s from a budget of 0.25 k: an exact 0.0."""
    out = []
    for k in _arrivals():
        for role, to in ROLES:
            out.append(World("P5-k%d-%s" % (k, role), [halted(0.0, 0.0, 0.25, t=_ulp(0.25 * k, to)), BYSTANDER],
                             Probe("P5-k%d" % k, role, "below", k - 1, 0, ("flag", F_RAN_OUT, "done"))))
    return out


# the centimetre bucket rint(gap * 100) at exact halves, from the definition of round-half-to-even (NOT from the oracle):
#   gap  0.125 -> 12.5 -> 12  (12 is even)      gap 0.375 -> 37.5 -> 38  (38 is even)
#   gap  0.625 -> 62.5 -> 62  (62 is even)      gap -0.125 -> -12.5 -> -12  (-12 is even; truncation gives -12 too, round-half-away -13)
# host H (agent 0, halted at the origin, goal on +x) sees X (agent 1, r 0.25) arrive on its goal axis from behind at that gap: lateral 0.
# Y (agent 2, r 0.375) stands straight below H (lateral < 0) in the bucket BELOW the half, Z (agent 3, r 0.5) straight above (lateral > 0)
# in the bucket ABOVE it.  Far to near is bucket descending, then lateral ascending, so
#   X rounded down (X shares Y's bucket; Z is further):  Z, Y, X          X rounded up (X shares Z's bucket):  X, Z, Y
HALVES = {0.125: (12, 13, "down"), 0.375: (37, 38, "up"), 0.625: (62, 63, "down"), -0.125: (-13, -12, "up")}
P6_ORDER = {"down": (3, 2, 1), "up": (1, 3, 2)}
P6_NEG_ORDER = {"down": (3, 2, 1), "up": (3, 1, 2)}


def p6_halves():
    out = []
    for half, (lo, hi, way) in sorted(HALVES.items()):
        for k in _arrivals():
            for role, to in ROLES:
                rh = 0.25
                x_end = -(half + rh + 0.25)                     # X's centre when it has arrived: |x_end| - 0.25 - 0.25 = half, exactly
                x0 = _ulp(x_end - 0.25 * k, None if to is None else -to)    # (an ulp further LEFT is an ulp more gap)
                y = static(0.0, -(lo / 100.0 + rh + 0.375), 0.375)
                if half > 0:
                    agents, orders = [halted(0.0, 0.0, rh), mover(x0, 0.0, 0.25), y, static(0.0, hi / 100.0 + rh + 0.5, 0.5)], P6_ORDER
                else:
                    # overlapping: X collides when it arrives and H with Y from the first step on -- H is a static agent here (its row is
                    # observed like a learner's) and the bystander takes Z's place (four agents must do): it is the farthest, then
                    # Y, X (X rounded down into Y's bucket) or X, Y (rounded up, out of it)
                    agents, orders = [static(0.0, 0.0, rh, True), mover(x0, 0.0, 0.25), y, BYSTANDER], P6_NEG_ORDER
                order = orders[way] if to is None else orders["down" if role == "below" else "up"]
                out.append(World("P6-%g-k%d-%s" % (half, k, role), agents,
                                 Probe("P6-%g-k%d" % (half, k), role, "below" if way == "down" else "above", k - 1, 0, ("slots",)), None, order))
    return out


def p7_tti():
    """P7  time_to_impact's branches (sort_method 2; far to near is tti descending, then the bucket descending, then the lateral).
    touch   c == 0: H (r 0.25) arrives touching X (r 0.5, ahead on the axis) and Y (r 0.375, straight below): both tti 0, bucket 0, Y's
            lateral is smaller -> Y, X.  X one ulp further: c > 0, tti = 1 ulp > 0 -> X, Y.
    static  a == 0: H halted, X static -> inf; Y moves at H head on... (Y behind H on the axis, moving at it: finite) -> X, Y.  Not taken:
            H moves at half speed towards X, which then has the smaller finite tti -> Y, X.
    perp    b == 0: H moves along x, X exactly beside it after the move -> inf -> X, Y (Y ahead on the axis, finite).  Not taken: X
            0.75 ahead of that, the ray hits it (tti < Y's) -> Y, X.
    graze   rx = 0.5, ry = 1, R = 1, v = (1, 0): disc == 0, tti = 0.5; Y ahead on the axis at tti 2.375 -> Y, X.  ry one ulp more: disc < 0,
            inf -> X, Y.  (Not rx = 2: there rx^2 + ry^2 = 5 has an ulp of 2^-50 and swallows the 2^-51 that one ulp of ry adds -- the
            triple would not straddle in float64.  At rx = 0.5 the sum is 1.25 + 2^-51, exact.)"""
    out = []
    for k in _arrivals():
        x0 = -0.25 * k
        for role, to in ROLES:
            out.append(World("P7-touch-k%d-%s" % (k, role), [mover(x0, 0.0, 0.25), static(_ulp(0.75, to), 0.0, 0.5), static(0.0, -0.625, 0.375), BYSTANDER],
                             Probe("P7-touch-k%d" % k, role, "below", k - 1, 0, ("slots",))))
            out.append(World("P7-graze-k%d-%s" % (k, role), [mover(x0, 0.0, 0.5), static(0.5, _ulp(1.0, to), 0.5), static(3.25, 0.0, 0.375), BYSTANDER],
                             Probe("P7-graze-k%d" % k, role, "below", k - 1, 0, ("slots",))))
        # the branch taken ('at') and not taken ('above'): no ulp changes a == 0 or b == 0 into a hit
        y_from_behind = mover(-3.0 + x0, 0.0, 0.375)          # moves at H along the axis: finite tti at every step
        out.append(World("P7-static-k%d-at" % k, [halted(0.0, 0.0, 0.25), static(1.5, 0.0, 0.5), y_from_behind, BYSTANDER],
                         Probe("P7-static-k%d" % k, "at", None, k - 1, 0, ("slots",))))
        out.append(World("P7-static-k%d-above" % k, [mover(-0.125 * k, 0.0, 0.25, pref=0.5), static(1.5, 0.0, 0.5), y_from_behind, BYSTANDER],
                         Probe("P7-static-k%d" % k, "above", None, k - 1, 0, ("slots",))))
        out.append(World("P7-perp-k%d-at" % k, [mover(x0, 0.0, 0.25), static(0.0, 1.5, 0.5), static(4.0, 0.0, 0.375), BYSTANDER],
                         Probe("P7-perp-k%d" % k, "at", None, k - 1, 0, ("slots",))))
        out.append(World("P7-perp-k%d-above" % k, [mover(x0, 0.0, 0.25), static(1.5, 0.25, 0.5), static(4.0, 0.0, 0.375), BYSTANDER],
                         Probe("P7-perp-k%d" % k, "above", None, k - 1, 0, ("slots",))))
    return out


def p8_pi(closed):
    """P8  a turn to exactly +pi and to exactly -pi from heading 0 (table entries [1.0, +-pi], actions_fp32 = 0), after k - 1 straight
    moves.  wrap_closed_end = 0 wraps to [-pi, pi): both end at -pi; = 1 to (-pi, pi]: both end at +pi.  One ulp inside / outside."""
    out = []
    side = "below" if closed else "above"
    for k in _arrivals():
        for sign, turns in ((1, (TURN_PI_LO, TURN_PI, TURN_PI_HI)), (-1, (TURN_MPI_HI, TURN_MPI, TURN_MPI_LO))):
            for (role, _), turn in zip(ROLES, turns):
                act = (STRAIGHT,) * (k - 1) + (turn,) + (STOP,) * (STEPS - k)
                out.append(World("P8-%s-k%d-%s" % ("plus" if sign > 0 else "minus", k, role), [mover(0.0, 0.0, 0.25, act=act), BYSTANDER],
                                 Probe("P8-%s-k%d" % ("plus" if sign > 0 else "minus", k), role, side, k - 1, 0, ("hsign",))))
    return out


def p9_goal_floor():
    """P9  the goal-distance floor: the ego axes are normalised when dist_to_goal > 1e-8.  tx = 1e-8 exactly (the goal at 0, the agent at
    -1e-8: the float32 goal cannot hold 1e-8), ty = 0, a halted learner two metres ahead.  The row is read after observe() (step -1) and
    after zero-speed steps: the neighbour's p_parallel is 2.00000001 normalised and 2.00000001e-8 not."""
    out = []
    for role, tx in (("below", np.nextafter(1e-8, 0.0)), ("at", 1e-8), ("above", np.nextafter(1e-8, 1.0))):
        host = Agent(-tx, 0.0, 0.0, 0.0, 0.25, 1.0, 0, 0.0, 50.0, STOP)
        for step in (-1, 2):
            out.append(World("P9-s%d-%s" % (step, role), [host, halted(2.0, 0.0, 0.5)], Probe("P9-s%d" % step, role, "below", step, 0, ("pprll",))))
    return out


# ---- sort ties ---------------------------------------------------------------------------------------------------------------------
R1, R2, R3 = 0.25, 0.25 + 2.0 ** -16, 0.25 + 2.0 ** -15         # distinct float32 radii 15 and 30 micrometres apart: one bucket, three identities
ALL = tuple(range(-1, STEPS))


def _swapped(world):
    """the same world with agents 1 and 2 exchanged: the same radii must come out in the same slots, so a rule that prefers the lower (or
    the higher) index among equal fast keys fails one of the two"""
    a = list(world.agents)
    a[1], a[2] = a[2], a[1]
    return [world._replace(name=world.name + "-swapped", agents=a)]


def t1_full(three=False, tag="T1"):
    """a full tie: H (halted at the origin, goal (5, 0)) sees (1, 0.8) and (-1, 0.8): the same distance, so the same bucket (the radii differ by
    micrometres), and ry * tx - rx * ty = 0.8 * 5 - rx * 0 bit for bit -> agent index decides.  three: a third on the first one's spot."""
    agents = [halted(0.0, 0.0, 0.25, gx=5.0), static(1.0, 0.8, R1), static(-1.0, 0.8, R2)] + ([static(1.0, 0.8, R3)] if three else [])
    return [World("%s-%s" % (tag, "three" if three else "two"), agents, None, Tie(0, (1, 2, 3) if three else (1, 2), ALL, "full"))]


def t2_cut():
    """T2  M = 2 < N - 1: far to near is (1, 2 tied), 3 -- the cut far_to_near[-2:] falls between the tied 1 and 2: agent 2 is kept, 1 not."""
    agents = [halted(0.0, 0.0, 0.25, gx=5.0), static(1.0, 0.8, R1), static(-1.0, 0.8, R2), static(0.0, -1.0, 0.375)]
    return [World("T2-cut", agents, None, Tie(0, (1, 2), ALL, "full"))]


def t4_f32_lateral():
    """T4  laterals 1.0 + 2^-40 (agent 1) and 1.0 (agent 2) times the goal distance 5: the same float32, different float64 -> the smaller
    lateral first: 2, 1 -- against the index order."""
    agents = [halted(0.0, 0.0, 0.25, gx=5.0), static(1.0, 1.0 + 2.0 ** -40, R1), static(-1.0, 1.0, R2)]
    world = World("T4-f32-lateral", agents, None, Tie(0, (1, 2), ALL, "f32"))
    return [world] + _swapped(world)


def t5_exact_gap():
    """T5  sort_round_gap = 0.  (5, 12, 13) / 8 and (9, 12, 15) / 8: centre distances 1.625 and 1.875 with lateral 1.5, radii 0.25 and 0.5:
    float64 gaps of exactly 1.125 both (bit-equal) -- the lateral decides (agent 2 below the axis: -1.5 first, against the index order);
    agent 2 moved up by 2^-40 instead: the float32 gaps are equal, the float64 gaps are not -- the larger gap (agent 2) first although its
    lateral is the larger."""
    h = halted(0.0, 0.0, 0.25, gx=5.0)
    both = [World("T5-gap-bit-equal", [h, static(0.625, 1.5, 0.25), static(-1.125, -1.5, 0.5)], None, Tie(0, (1, 2), ALL, "gap64")),
            World("T5-gap-f32-equal", [h, static(0.625, 1.5, 0.25), static(-1.125, 1.5 + 2.0 ** -40, 0.5)], None, Tie(0, (1, 2), ALL, "gap32"))]
    return both + _swapped(both[0]) + _swapped(both[1])


def t7_persists():
    """T7  H halted with its goal on +y; the pair starts at (0.75, +-1) and moves along +x at the same speed: rx equal, ry mirrored -- the
    same distance and the same lateral -rx * ty at every step of the launch."""
    agents = [halted(0.0, 0.0, 0.25, gx=0.0, gy=5.0), mover(0.75, 1.0, R1), mover(0.75, -1.0, R2)]
    return [World("T7-persists", agents, None, Tie(0, (1, 2), ALL, "full"))]


def t8_appears():
    """T8  the same pair, agent 1 at half speed from x = 0.75, agent 2 at full speed from 0.375: after the third step both are at 1.125 --
    and at no other step."""
    agents = [halted(0.0, 0.0, 0.25, gx=0.0, gy=5.0), mover(0.75, 1.0, R1, pref=0.5), mover(0.375, -1.0, R2)]
    return [World("T8-appears", agents, None, Tie(0, (1, 2), (2,), "full"))]


def line(N):
    """all N agents present on the host's goal axis, the host (agent N // 2, halted) between them: the others in pairs at -+1, -+2, .. m,
    lateral 0 all, the radii 2^-14 apart (every pair in one bucket): N // 2 - 1 full ties, decided by the AGENT index -- which is not the
    ring order other_index() visits them in from a host in the middle."""
    h = N // 2
    others = [i for i in range(N) if i != h]
    agents = [None] * N
    agents[h] = halted(0.0, 0.0, 0.25)
    pairs = []
    for m, i in enumerate(others):
        agents[i] = static((1.0 + m // 2) * (1 if m % 2 == 0 else -1), 0.0, 0.25 + i * 2.0 ** -14)
        if m % 2 == 1:
            pairs.append((others[m - 1], i))
    return [World("line-%d" % N, agents, None, Tie(h, tuple(pairs[0]), ALL, "full") if pairs else None)]


def _passed_through():
    """U4 flipped decides: P1's k = 4 worlds with the static agent AT its goal (done from the first step on): the mover passes through it"""
    return [w._replace(name="U4-" + w.name, probe=None) for w in p1_collision(0.0) if "-k4-" in w.name]


TIES = lambda: t1_full() + t1_full(True) + t4_f32_lateral() + t7_persists() + t8_appears()

# ---- the groups ----------------------------------------------------------------------------------------------------------------------
# name -> (cavoid_cfg overrides beside BASE, M (None: N - 1), the worlds)
Group = collections.namedtuple("Group", "name over M worlds")


def _groups():
    g = [
        Group("main", dict(), None, p1_collision(0.0) + p2_close() + p4_goal() + p5_timeout() + p6_halves() + p9_goal_floor() + TIES()),
        Group("cd25", dict(collision_dist=0.25), None, p1_collision(0.25) + t1_full()),
        Group("horizon", dict(sensing_horizon=1.25), None, p3_horizon()),
        Group("m2", dict(), 2, t2_cut() + t1_full(True) + t7_persists()),
        Group("near", dict(sort_method=1), None, TIES() + t2_cut()),                     # T3: closest_first re-ranks the kept set
        Group("near-m2", dict(sort_method=1), 2, t2_cut() + t1_full(True) + t7_persists()),
        Group("tti", dict(sort_method=2), None, p7_tti() + TIES()),
        Group("exact-gap", dict(sort_round_gap=0), None, t5_exact_gap() + TIES()),       # T5
        Group("index-tie", dict(sort_tie_lateral=0), None, TIES() + t2_cut()),           # T6
        Group("pi-open", dict(wrap_closed_end=0, actions_fp32=0, actions=PI_TABLE), None, p8_pi(False)),
        Group("pi-closed", dict(wrap_closed_end=1, actions_fp32=0, actions=PI_TABLE), None, p8_pi(True)),
        Group("u4", dict(done_agents_collide=0), None, p1_collision(0.0, True) + p2_close(True) + _passed_through() + t1_full()),
        Group("u4-cd25", dict(done_agents_collide=0, collision_dist=0.25), None, p1_collision(0.25, True)),
    ]
    return collections.OrderedDict((x.name, x) for x in g)


GROUPS = _groups()


def over_of(group):
    return dict(BASE, **group.over)


def worlds_of(group, N):
    """the group's worlds at N agents per world: those that fit (every hand-placed world has at most 4 agents) and the line of N"""
    return [w for w in group.worlds if len(w.agents) <= N] + line(N)


# worlds per batch: the shapes whose launch forms tests/test_gpu_cfg_fields.py::HORIZON_FORMS and cfg_regimes.CROWD_SHAPES name
WORLDS = {4: 512, 5: 256, 6: 256, 10: 300, 16: 256, 17: 250, 33: 231, 64: 220}


def num_worlds(group, N):
    return max(WORLDS.get(N, 0), STRIDE * len(worlds_of(group, N)) + 1)


def world_index(k):
    return STRIDE * k + 1


def M_of(group, N):
    return N - 1 if group.M is None else min(group.M, N - 1)


def oracle_for(group, N):
    return rp.oracle_for(N, M_of(group, N), **over_of(group))


def place(group, N, st):
    """write the group's worlds over generator worlds of `st` (co.State of num_worlds(group, N) worlds): state as set_state takes it"""
    for k, w in enumerate(worlds_of(group, N)):
        base = world_index(k) * N
        sl = slice(base, base + N)
        st.f64[:, sl], st.f32[:, sl], st.flags[sl] = 0.0, 0.0, 0
        for i, a in enumerate(w.agents):
            st.f64[:, base + i] = (a.px, a.py, a.heading, a.t)
            st.f32[:, base + i] = (a.gx, a.gy, a.r, a.pref, 0.0)
            st.flags[base + i] = F_PRESENT | (F_LEARNING if a.pol == 0 else 0) | (a.pol << 8)
            assert float(np.float32(a.r)) == a.r and float(np.float32(a.pref)) == a.pref, w.name


def actions(group, N, W):
    """int32 [STEPS, W, N]: the placed agents' own actions; generator worlds go straight ahead"""
    acts = np.full((STEPS, W, N), STRAIGHT, np.int32)
    for k, w in enumerate(worlds_of(group, N)):
        for i, a in enumerate(w.agents):
            acts[:, world_index(k), i] = a.act
    return acts


class Run(object):
    """the C oracle over one group at N agents: generator worlds from the reset, the hand-placed ones written over every third, the
    observation of the pushed state and STEPS auto-reset steps -- computed once, shared by the tests of a session and never changed"""
    _cache = {}

    def __init__(self, group, N, straight=False):
        """straight: every agent is given the straight-ahead action at every step (what a closed actor loop on a network with a constant
        greedy action gives its learners: the halted agents then move too -- the movers' thresholds and the moving ties stay as they are)"""
        self.group, self.N, self.W = group, N, num_worlds(group, N)
        self.cfg, self.gen = oracle_for(group, N)
        st = co.State.empty(self.W, N)
        self.ep = np.zeros(self.W, np.uint32)
        co.generate(self.cfg, self.gen, SEED, st, self.ep)
        place(group, N, st)
        self.start = st.copy()
        self.acts = np.full((STEPS, self.W, N), STRAIGHT, np.int32) if straight else actions(group, N, self.W)
        self.obs0 = co.observe(self.cfg, st)
        self.outs, self.states, self.eps = [], [], []
        for t in range(STEPS):
            self.outs.append(co.step_autoreset(self.cfg, self.gen, SEED, st, self.ep, self.acts[t]))
            self.states.append(st.copy())
            self.eps.append(self.ep.copy())

    @classmethod
    def of(cls, name, N, straight=False):
        key = (name, N, straight)
        if key not in cls._cache:
            cls._cache[key] = cls(GROUPS[name], N, straight)
        return cls._cache[key]

    def worlds(self):
        return list(enumerate(worlds_of(self.group, self.N)))

    def row(self, k, step, host):
        """the host's observation row of hand-placed world k after step `step` (-1: of the pushed state)"""
        return (self.obs0 if step < 0 else self.outs[step][0])[world_index(k), host]

    def state(self, step):
        return self.start if step < 0 else self.states[step]


def slot_radii(row, M):
    """the float32 radius column of a row's slots: WHO sits in each slot (every placed agent has its own radius)"""
    return tuple(np.asarray(row[6 + 4:6 + 7 * M:7], np.float32).tolist())


def read(run, k, probe, outs=None, states=None, obs0=None):
    """the decisive quantity of a probe, from the oracle run or (outs / states / obs0 given: the same structures) from a subject"""
    outs = run.outs if outs is None else outs
    states = run.states if states is None else states
    obs0 = run.obs0 if obs0 is None else obs0
    w, N, M = world_index(k), run.N, M_of(run.group, run.N)
    a = w * N + probe.host
    row = (obs0 if probe.step < 0 else outs[probe.step][0])[w, probe.host]
    got, it = [], iter(probe.read)
    for what in it:
        if what == "flag":
            got.append(bool(states[probe.step].flags[a] & next(it)))
        elif what == "rew":
            got.append(round(float(outs[probe.step][1][w, probe.host]), 6))
        elif what == "done":
            got.append(int(outs[probe.step][2][w, probe.host]))
        elif what == "nobs":
            got.append(float(row[1]))
        elif what == "slots":
            got.append(slot_radii(row, M))
        elif what == "hsign":
            got.append(bool(np.signbit(states[probe.step].f64[2, a])))
        elif what == "pprll":
            got.append(float(row[6]) > 1.0)
    return tuple(got)


def expected_slots(world, order, M):
    """slot radii of `order` (agent indices, far to near) under closest_last with every neighbour kept"""
    r = [float(np.float32(world.agents[i].r)) for i in order]
    return tuple(r + [0.0] * (M - len(r)))
