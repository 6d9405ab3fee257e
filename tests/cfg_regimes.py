"""Shared cases of the tests that take the env step off the default numbers of `cavoid_cfg` (the pattern of tests/policy_regimes.py).
A plain module: tests/test_cfg_regimes_host.py (CPU, the float64 oracle alone) and the GPU tests -- tests/test_gpu_cfg_fields.py (tile
forms), tests/test_gpu_crowd_cfg.py (crowd form), tests/test_gpu_actor_oracle.py (the fused actor's env half) -- build the SAME cases
from it, so that what the host test proves about a case (every field decides something within the case's steps; restarts, collisions,
both clip ends, hidden neighbours really happen) holds for the batch the kernels run.

Step-side sets.  The clip hides the goal reward, so one set cannot show both:
  CLIPPED    every numeric field of the step off its default; both clip ends act (reward_at_goal 1.0 -> 0.7, reward_collision -0.5 -> -0.4);
  UNCLIPPED  the same with reward_at_goal = 0.8 inside a clip that never acts.
Both run with dynamics = 1 (unicycle_max_turn_rate) and the WIDE table, so that max_turn_rate * dt (2.0 * 0.1 = 0.2 rad) clamps.
Generator-side sets: RING (gen_mode 0) and BOX (gen_mode 1; the small boxes make placement rounds fail at high agent counts -- both
sides must give up the same way).  The values are not measurements; every field stays off its default."""
import collections

import numpy as np

from oracle import c_oracle as co
from tests import replay as rp

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
F_AT_GOAL, F_RAN_OUT, F_IN_COLL, F_PRESENT = 1, 2, 4, 0x20

# ---- action tables -----------------------------------------------------------------------------------------------------------
TABLE5 = [[1.0, 0.0], [1.0, np.pi / 6], [1.0, -np.pi / 6], [0.5, 0.0], [0.0, 0.0]]
# 32 actions are 64 doubles: in the crowd form every lane of the wavefront loads one table entry
TABLE32 = [[(1.0, 0.5, 0.0, 0.75)[k % 4], (k - 16) * np.pi / 40] for k in range(32)]
# turns beyond max_turn_rate * dt (3 rad/s * 0.2 s): the default table's widest turn (pi/6) never reaches the max-turn clamp
WIDE = [[1.0, 0.3], [1.0, -0.3], [1.0, 0.0], [1.0, 0.9], [1.0, -0.9], [0.5, 1.2], [0.5, -1.2], [0.0, 0.7], [0.0, -0.7], [1.0, 1.5], [1.0, -1.5]]

# ---- the sets -----------------------------------------------------------------------------------------------------------------
CLIPPED = dict(dt=0.1, near_goal_threshold=0.35, max_time_ratio=1.5, collision_dist=0.05, getting_close_range=0.4, reward_collision=-0.5,
               reward_getting_close=-0.05, reward_time_step=-0.01, close_penalty_slope=0.25, reward_clip_lo=-0.4, reward_clip_hi=0.7,
               max_turn_rate=2.0, sensing_horizon=4.0)
UNCLIPPED = dict(CLIPPED, reward_at_goal=0.8, reward_clip_lo=-1.0, reward_clip_hi=2.0)
STEP_SETS = {"CLIPPED": CLIPPED, "UNCLIPPED": UNCLIPPED}
MAX_TURN = dict(dynamics=1, actions=WIDE)              # beside either set
RING = dict(gen_goal_jitter=0.2, gen_angle_jitter=0.6, gen_static_fraction=0.8, gen_nonlearning_fraction=0.4, gen_min_agents=2)
BOX = dict(gen_mode=1, gen_box_small=(3.0, 3.5), gen_box_large=(5.0, 9.0), gen_box_large_from=4, gen_min_trip=2.5, gen_static_fraction=0.8,
           gen_nonlearning_fraction=0.4, gen_min_agents=2)
GEN_SETS = {"RING": RING, "BOX": BOX}
# cavoid_default_cfg's values of the sets' fields (gen_min_agents: the world size, see field_default)
DEFAULTS = dict(dt=0.2, near_goal_threshold=0.2, max_time_ratio=2.0, collision_dist=0.0, getting_close_range=0.2, reward_at_goal=1.0,
                reward_collision=-0.25, reward_getting_close=-0.1, reward_time_step=0.0, close_penalty_slope=0.5, reward_clip_lo=-0.25,
                reward_clip_hi=1.0, max_turn_rate=3.0, sensing_horizon=float("inf"),
                gen_goal_jitter=0.5, gen_angle_jitter=0.25, gen_static_fraction=0.5, gen_nonlearning_fraction=0.0, gen_box_small=(4.0, 5.0),
                gen_box_large=(6.0, 8.0), gen_box_large_from=5, gen_min_trip=1.0)
DEFAULT_POOL = 65536                                   # cavoid_default_cfg's gen_pool_size


def field_default(field, N):
    return N if field == "gen_min_agents" else DEFAULTS[field]


# ---- actions -----------------------------------------------------------------------------------------------------------------
def _goal_seeking_actions(rng, W, N, p_straight=0.8):
    """uniform random actions, biased to 'full speed straight ahead' (index 2) so that agents also
    REACH goals (pure noise mostly times out or collides)."""
    acts = rng.integers(0, 11, size=(W, N))
    acts[rng.random((W, N)) < p_straight] = 2
    return acts.astype(np.int32)


def _cont_actions(rng, dyn, st, K, W, N):
    """K slices of continuous actions [K,W,N,2]: holonomic = a velocity towards the goal (as seen from `st`) + noise, unicycle =
    (speed, heading change) with the heading change biased towards the goal so that agents also arrive"""
    g = np.stack([st.f32[0] - st.f64[0], st.f32[1] - st.f64[1]], -1).reshape(W, N, 2)
    if dyn == "holonomic":
        v = g / np.maximum(np.linalg.norm(g, axis=-1, keepdims=True), 1e-6) * st.f32[3].reshape(W, N, 1)
        return (v[None] + rng.normal(0, 0.3, size=(K, W, N, 2))).astype(np.float32)
    to_goal = np.arctan2(g[..., 1], g[..., 0]) - st.f64[2].reshape(W, N)
    to_goal = (to_goal + np.pi) % (2 * np.pi) - np.pi
    dh = np.clip(to_goal, -0.5, 0.5)[None] * (rng.random((K, W, N)) < 0.7) + rng.uniform(-0.4, 0.4, (K, W, N))
    sp = st.f32[3].reshape(1, W, N) * rng.uniform(0.3, 1.0, (K, W, N))
    return np.stack([sp, dh], -1).astype(np.float32)


def _edge_actions(rng, T, W, N, num_actions, straight, p_edge=0.03):
    """tests/test_gpu_launch_forms._actions: (raw, clamped) int32 [T, W, N], mostly straight ahead, some random, and a few out-of-range
    values of every kind in the raw set (cavoid.h: table actions are clamped; the oracle is handed them clamped)"""
    a = rng.integers(0, num_actions, size=(T, W, N)).astype(np.int64)
    a[rng.random((T, W, N)) < 0.6] = straight
    edge = rng.random((T, W, N)) < p_edge
    a[edge] = rng.choice(np.array([-1, num_actions, INT32_MIN, INT32_MAX], np.int64), size=int(edge.sum()))
    return a.astype(np.int32), np.clip(a, 0, num_actions - 1).astype(np.int32)


DYN_NAME = {0: "unicycle", 1: "unicycle_max_turn_rate", 2: "holonomic"}

# ---- the cases ---------------------------------------------------------------------------------------------------------------
# over: every cavoid_cfg override (both sides); fields: the set fields held by "every field decides something"; plan: the launches, in
# order, as (kind, slots, steps) with kind in single / slots / packed; acts: goal (goal-seeking table indices), edge (table indices with
# out-of-range values), cont (continuous); expect: the events the case must see; pipe: CAVOID_PIPELINE while the env is created
# offset: the env's world_offset (the generator is keyed on offset + world)
Case = collections.namedtuple("Case", "cid family N W seed over fields plan acts straight expect pipe forms offset", defaults=(0,))


def _numeric_plan(single, K, P):
    return (("single", 1, 1),) * single + (("slots", K, K), ("packed", P, P))


NUMERIC_EVENTS = ("restart", "collision", "close", "horizon", "time_step")


def _numeric(cid, family, N, W, seed, step_set, gen_set, source, plan, pipe=None, forms=None):
    over = dict(STEP_SETS[step_set], **MAX_TURN)
    over.update(GEN_SETS[gen_set])
    over.update(source)
    fields = dict(STEP_SETS[step_set], **GEN_SETS[gen_set])
    fields.pop("gen_mode", None)                       # a switch, not a number: RING and BOX are its two values
    # by construction reward_at_goal decides nothing under CLIPPED (1.0 and any other value above reward_clip_hi are paid as 0.7) and
    # reward_clip_hi nothing under UNCLIPPED (no reward reaches 1.0, its default): each is held by the other set
    fields.pop("reward_at_goal" if step_set == "CLIPPED" else "reward_clip_hi", None)
    expect = NUMERIC_EVENTS + (("clip_lo", "clip_hi") if step_set == "CLIPPED" else ())
    return Case(cid, family, N, W, seed, over, fields, plan, "goal", 2, expect, pipe, forms)


# the tile forms (tests/test_gpu_cfg_fields.py): (N, W, pipe, gen set, scenario source) -> (form of one step per launch, form of the K-step
# launch).  dynamics = 1 changes no form: QUAD refuses only the holonomic dynamics, the relay carries the max-turn clamp.  Box scenarios
# generated inside the step (gen_mode = 1 without a pool) go to the 'everything' instantiations of env_kernel whatever the batch and the
# switch (RVO: the only ones with the cooperative placement compiled in), one step per launch and in the step loop alike.
TILE_SHAPES = [
    ("n4-relay-ring-pool", 4, 512, None, "RING", dict(), ("QUAD", ("RELAY", 3))),
    ("n4-pipe-ring-lookahead", 4, 512, "1", "RING", dict(gen_pool_size=0, gen_lookahead=64), ("QUAD", ("PIPE", 0))),
    ("n4-looppf-ring-pool500", 4, 512, "0", "RING", dict(gen_pool_size=500), ("QUAD", ("LOOP_PF", 0))),
    ("n4-nopipe-box-instep", 4, 512, "0", "BOX", dict(gen_pool_size=0), ("RVO", ("RVO", 0))),
    ("n4-40000-loop-ring-pool", 4, 40000, None, "RING", dict(), ("STEP", ("LOOP", 0))),     # beyond latency mode: the plain loop
    ("n10-box-instep", 10, 300, None, "BOX", dict(gen_pool_size=0), ("RVO", ("RVO", 0))),
]
TILE_SEED = 29
# the crowd form (tests/test_gpu_crowd_cfg.py): the smallest shapes at which the lane mapping differs
CROWD_SHAPES = [(17, 50), (24, 65), (33, 33), (64, 20)]      # 3 worlds per wavefront (ragged last) / 2 / 1 with 31 idle lanes / all lanes
CROWD_SEED = 8
# gen_box_large_from decides only in worlds of exactly 4 agents: with 2..64 agents per world 20 worlds draw none
CROWD_BOX_WORLDS = {33: 66, 64: 120}


def _cases():
    out = []
    for step_set in ("CLIPPED", "UNCLIPPED"):
        for tag, N, W, pipe, gen_set, source, forms in TILE_SHAPES:
            plan = _numeric_plan(30, 16, 6) if W > 10000 else _numeric_plan(140, 40, 8)
            out.append(_numeric("tile-%s-%s" % (step_set.lower(), tag), "tile", N, W, TILE_SEED, step_set, gen_set, source, plan, pipe, forms))
        for N, W in CROWD_SHAPES:
            out.append(_numeric("crowd-%s-ring-pool-%dx%d" % (step_set.lower(), N, W), "crowd", N, W, CROWD_SEED, step_set, "RING",
                                dict(gen_pool_size=200), _numeric_plan(140, 20, 5)))
            Wb = CROWD_BOX_WORLDS.get(N, W)
            out.append(_numeric("crowd-%s-box-instep-%dx%d" % (step_set.lower(), N, Wb), "crowd", N, Wb, CROWD_SEED, step_set, "BOX",
                                dict(gen_pool_size=0), _numeric_plan(140, 20, 5)))
    # the fused actor's env half (tests/test_gpu_actor_oracle.py draws its own actions: the host test runs the configuration with
    # goal-seeking ones over the same number of steps)
    out.append(_numeric("actor-unclipped-ring-4x256", "tile", 4, 256, 33, "UNCLIPPED", "RING", dict(), (("single", 1, 1),) * 92))
    # ---- crowd form, continuous actions: 50 single steps, then K = 16 launches in slots (one shorter than its slots) and packed ----
    cont_plan = (("single", 1, 1),) * 50 + (("slots", 16, 16),) * 3 + (("slots", 16, 11),) + (("slots", 16, 16),) * 3 + (("packed", 16, 16),) * 3
    base = dict(gen_min_agents=2, gen_nonlearning_fraction=0.3)
    for dyn in (0, 1, 2):
        for (N, W), source in (((17, 50), dict(gen_pool_size=200)), ((24, 65), dict(gen_pool_size=0))):
            out.append(Case("crowd-cont-%s-%dx%d" % (DYN_NAME[dyn], N, W), "crowd", N, W, 23, dict(base, dynamics=dyn, **source), {}, cont_plan,
                            "cont", None, ("restart", "restart_share"), None, None))
    out.append(Case("crowd-cont-holonomic-box-instep-33x33", "crowd", 33, 33, 23, dict(base, dynamics=2, gen_mode=1, gen_pool_size=0), {},
                    cont_plan, "cont", None, ("restart", "restart_share"), None, None))
    # (with the default time budget 64-agent worlds hardly ever end within the case's steps)
    out.append(Case("crowd-cont-unicycle-budget-64x20", "crowd", 64, 20, 23, dict(base, dynamics=0, max_time_ratio=0.3, gen_pool_size=200), {},
                    cont_plan, "cont", None, ("restart", "restart_share"), None, None))
    # ---- crowd form, table actions: other tables, out-of-range indices ------------------------------------------------------------
    table_plan = _numeric_plan(140, 20, 5)
    for tag, N, W, over, straight in (("max-turn-wide", 20, 65, dict(MAX_TURN), 2), ("table5", 22, 65, dict(actions=TABLE5), 0),
                                      ("table32", 33, 33, dict(actions=TABLE32), 16), ("table32", 64, 20, dict(actions=TABLE32), 16)):
        out.append(Case("crowd-%s-%dx%d" % (tag, N, W), "crowd", N, W, 42, dict(base, gen_pool_size=200, **over), {}, table_plan, "edge", straight,
                        ("restart", "collision"), None, None))
    # ---- crowd form, restart pressure: a time budget of one step, 40 steps -----------------------------------------------------
    press_plan = _numeric_plan(20, 15, 5)
    for tag, N, W, source in (("pool", 20, 65, dict(gen_pool_size=200)), ("box-instep", 33, 33, dict(gen_mode=1, gen_pool_size=0)),
                              ("ring-instep", 64, 20, dict(gen_pool_size=0))):
        out.append(Case("crowd-pressure-%s-%dx%d" % (tag, N, W), "crowd", N, W, 7, dict(base, max_time_ratio=0.01, **source), {}, press_plan, "goal", 2,
                        ("restart", "every_world_restarts"), None, None))
    return out + _topup_cases()


# ---- the relay launch's ring top-up (tests/test_gpu_topup_oracle.py) -----------------------------------------------------------------
# Look-ahead rings of R records per world, GEN v1 generated (gen_pool_size = 0), and nothing but K-step launches with K <= R / 2 behind the
# reset: the first fill (ahead_fill_kernel) makes the records of episodes 1 .. R, every later record is made by the top-up wavefront of an
# earlier relay launch (csrc/cavoid_relay.hpp, relay_topup).  A time budget of 0.03 x the straight-line time ends an episode every four or five
# steps, at different steps in different worlds, so that within a case's steps EVERY world reads records three rings deep (`ring_turnover`):
# records only the role can have made, from its own copy of the generator fields (RING, off their defaults), of max_time_ratio and of
# world_offset.  No goal is reached under this budget: the goal-side step fields stay with the tile- cases.
TOPUP_SEED = 11
TOPUP_RATIO = 0.03
UNICYCLE = dict(dynamics=0)                            # the plain unicycle on the default table of 11 actions (straight ahead at index 2 too)


def _topup(tag, N, W, step_set, kinds, R=8, K=4, launches=48, ratio=TOPUP_RATIO, dyn=MAX_TURN, offset=0, exempt=(), **gen_over):
    over = dict(STEP_SETS[step_set], **dyn)
    over.update(RING)
    over.update(gen_over)
    over.update(max_time_ratio=ratio, gen_pool_size=0, gen_lookahead=R)
    # what the role's own loads must carry (tests/test_cfg_regimes_host.py: each decides something in episodes above R).  By construction
    # gen_min_agents decides nothing where it equals the world size (its default), and a world of one agent draws no policy (agent 0 always
    # learns): gen_static_fraction and gen_nonlearning_fraction decide nothing at N = 1
    fields = dict(RING, max_time_ratio=ratio, **gen_over)
    if fields["gen_min_agents"] == N:
        del fields["gen_min_agents"]
    if N == 1:
        del fields["gen_static_fraction"], fields["gen_nonlearning_fraction"]
    plan = tuple((kinds[l % len(kinds)], K, K) for l in range(launches))
    expect = tuple(e for e in ("restart", "collision", "staggered", "ring_turnover") if e not in exempt)
    return Case("topup-" + tag, "topup", N, W, TOPUP_SEED, over, fields, plan, "goal", 2, expect, None, ("QUAD", "RELAY"), offset)


def _topup_cases():
    both = ("slots", "packed")
    return [
        _topup("clipped-n4x40", 4, 40, "CLIPPED", both),                            # 16 worlds per tile: a ragged last tile
        _topup("unclipped-n5x33", 5, 33, "UNCLIPPED", ("packed",)),
        _topup("clipped-n3x45", 3, 45, "CLIPPED", ("slots",), gen_min_agents=1),      # 21 worlds per tile, one idle lane, ragged
        _topup("clipped-n2x33", 2, 33, "CLIPPED", ("slots",)),
        # (a lone agent collides with nobody; the oracle's generator divides by zero if min_agents > N)
        _topup("clipped-n1x70", 1, 70, "CLIPPED", ("slots",), exempt=("collision",), gen_min_agents=1),
        _topup("clipped-n4x40-offset300", 4, 40, "CLIPPED", ("slots",), offset=300),  # (not a multiple of the tile's 16 worlds)
        # the relay decodes table actions only (cavoid_relay.hip refuses io.cont, and the holonomic dynamics take nothing else: a continuous
        # K-step launch runs the single-wavefront loop behind refill launches and never the role).  In place of continuous holonomic /
        # unicycle cases at these shapes: the nearest configuration the relay carries, the plain unicycle (dynamics 0, which no other topup-
        # case runs) on the default action table, per-step slots and packed records
        _topup("unicycle-table-n4x40", 4, 40, "UNCLIPPED", both, dyn=UNICYCLE),
        _topup("unicycle-table-n3x45", 3, 45, "CLIPPED", both, dyn=UNICYCLE, gen_min_agents=1),
        # the benchmark's ring: one-step episodes, every world restarts at every step and every slot is regenerated and read.  6 launches,
        # not 5: 3 R = 384 episodes.  (Collisions: gen_angle_jitter = 0.6 starts neighbours on top of each other.)
        _topup("ring128-n4x40", 4, 40, "CLIPPED", both, R=128, K=64, launches=6, ratio=1e-9, exempt=("staggered",)),
    ]


CASES = _cases()
BY_ID = {c.cid: c for c in CASES}
assert len(BY_ID) == len(CASES)


def select(prefix):
    return [c for c in CASES if c.cid.startswith(prefix)]


def steps_of(case):
    return sum(n for _, _, n in case.plan)


def num_actions(case):
    return len(case.over.get("actions", ())) or 11


def oracle_for(case, **changed):
    """(OracleCfg, OracleGen) of the case, `changed` fields replaced"""
    return rp.oracle_for(case.N, None, **dict(case.over, **changed))


def clip(cfg, r):
    return min(max(r, cfg.reward_clip_lo), cfg.reward_clip_hi)


class OracleRun(object):
    """The float64 oracle on one case: reset, then the case's launches.  `draw(K)` hands out the next K action slices as (what the env is
    given, what the oracle is given); `step(fed)` advances one step and notes the events in `seen`."""

    def __init__(self, case, start_episode=None, **changed):
        """start_episode (uint32 [W]): the per-world counters the env is seeded with (`env.seed(seed, episode)`); the reset starts the next"""
        self.case = case
        self.cfg, self.gen = oracle_for(case, **changed)
        self.st = co.State.empty(case.W, case.N)
        self.ep0 = np.zeros(case.W, np.uint32) if start_episode is None else np.asarray(start_episode, np.uint32) + np.uint32(1)
        self.ep = self.ep0.copy()
        co.generate(self.cfg, self.gen, case.seed, self.st, self.ep, world_offset=case.offset)
        self.rng = np.random.default_rng(case.seed)
        self.seen = collections.Counter()
        self.t = 0

    def draw(self, K):
        c = self.case
        if c.acts == "cont":
            a = _cont_actions(self.rng, DYN_NAME[c.over.get("dynamics", 0)], self.st, K, c.W, c.N)
            return a, a
        if c.acts == "edge":
            return _edge_actions(self.rng, K, c.W, c.N, num_actions(c), c.straight)
        a = np.stack([_goal_seeking_actions(self.rng, c.W, c.N) for _ in range(K)])
        return a, a

    def step(self, fed):
        c, cfg, st = self.case, self.cfg, self.st
        out = co.step_autoreset(cfg, self.gen, c.seed, st, self.ep, None if c.acts == "cont" else fed, world_offset=c.offset,
                                cont=fed if c.acts == "cont" else None)
        obs, rew, done, go = out
        self.t += 1
        s = self.seen
        present = (st.flags.reshape(c.W, c.N) & F_PRESENT) != 0         # (a restarted world: its new episode, as in the observation)
        n_world = present.sum(axis=1, keepdims=True)
        s["restart"] += int(go.sum())
        s["staggered"] += int(0 < int(go.sum()) < c.W)                  # some worlds restart at this step and some do not
        r_goal, r_coll, r_step = clip(cfg, cfg.reward_at_goal), clip(cfg, cfg.reward_collision), cfg.reward_time_step
        s["goal"] += int((rew == r_goal).sum())
        s["collision"] += int((rew == r_coll).sum())
        s["timeout"] += int((st.flags & F_RAN_OUT != 0).sum())           # (seen in worlds that run on: another learner is still on its way)
        if r_step != 0.0:
            s["time_step"] += int((rew == r_step).sum())
            s["close"] += int(((rew != 0.0) & (rew != r_goal) & (rew != r_coll) & (rew != r_step)).sum())
        s["clip_lo"] += int((rew == cfg.reward_clip_lo).sum())
        s["clip_hi"] += int((rew == cfg.reward_clip_hi).sum())
        visible = np.minimum(np.broadcast_to(n_world - 1, present.shape), cfg.max_other)
        s["horizon"] += int((obs[..., 1][present] < visible[present]).sum())
        return out

    def restart_share(self):
        return float((self.ep >= 1).mean())

    def turns(self):
        """episodes every world has started since the reset (uint32: the counters may wrap)"""
        return self.ep - self.ep0


# conditions, not measurements: the share of worlds that restarted within a continuous-action case's steps
MIN_RESTART_SHARE = {17: 0.3, 24: 0.3, 33: 0.2, 64: 0.2}


def assert_events(case, run):
    """what the case must have seen by its last step; if a seed or a step count misses one, another is picked -- the condition stays"""
    for ev in case.expect:
        if ev == "restart_share":
            assert run.restart_share() >= MIN_RESTART_SHARE[case.N], (case.cid, ev, run.restart_share())
        elif ev == "every_world_restarts":
            assert run.ep.min() >= 1, (case.cid, ev)
        elif ev == "ring_turnover":                             # every world has read records that only a top-up launch can have made
            assert run.turns().min() >= 3 * case.over["gen_lookahead"], (case.cid, ev, int(run.turns().min()))
        else:
            assert run.seen[ev] > 0, (case.cid, ev, dict(run.seen))


def run_oracle(case):
    run = OracleRun(case)
    for kind, K, n in case.plan:
        _, fed = run.draw(K)
        for t in range(n):
            run.step(fed[t])
    return run


# ---- the GPU side: one env through the case's launches, every step against the oracle ----------------------------------------------
OBS_TOL, STATE_TOL, GEN_TOL = 1e-5, 1e-9, 1e-12


def _assert_outputs(tag, obs, rew, done, go, ora):
    oobs, orew, odone, ogo = ora
    assert np.array_equal(done, odone) and np.array_equal(go, ogo), tag
    assert float(np.abs(rew - orew).max()) <= OBS_TOL, (tag, float(np.abs(rew - orew).max()))
    d = rp.obs_diff(obs, oobs)                                  # (the ego heading on the circle)
    assert float(d.max()) <= OBS_TOL, (tag, float(d.max()))
    assert np.array_equal(obs[..., :2], oobs[..., :2].astype(np.float32)), tag     # is_learning, num_other_agents exact


def _assert_state(tag, env, run, f64_tol=STATE_TOL):
    f64, f32, fl = [v.cpu().numpy() for v in env.get_state()]
    assert np.array_equal(fl.view(np.uint32), run.st.flags), tag                   # every flag bit
    assert np.array_equal(f32, run.st.f32), tag
    assert float(np.abs(f64 - run.st.f64).max()) <= f64_tol, (tag, float(np.abs(f64 - run.st.f64).max()))
    assert np.array_equal(env.episode.cpu().numpy().view(np.uint32), run.ep), tag


def _form_is(env, want):
    """`want`: (form, relay consumers) -- compared whole -- or the form's name alone, which leaves the consumer count UNCHECKED: only for a
    caller that does not fix the count (the topup- cases run whatever CAVOID_RELAY_CONSUMERS' default gives; the consumer-count test passes
    the tuple)"""
    got = env.last_step_form
    return got[0] == want if isinstance(want, str) else got == want


def _same_bits(tag, env, twin, outs, twin_outs):
    import torch
    assert all(torch.equal(a, b) for a, b in zip(outs, twin_outs)), tag
    assert all(torch.equal(a, b) for a, b in zip(env.get_state(), twin.get_state())) and torch.equal(env.episode, twin.episode), tag


def drive_plan(case, env, run, plan, single_form, k_form, twin=None, twin_form=None, after_launch=None):
    """the launches of `plan` on `env` beside the oracle run `run` (drive_gpu's checks).  `twin`: a second env taken through the same
    launches and held BITWISE to `env` -- every output of every step, state and episodes after every launch (twin_form: the form of its
    K-step launches where that is asserted too).  after_launch(launch index): called behind every launch's checks."""
    import torch
    cont = case.acts == "cont"
    wdt = env.obs_width
    slots = {}

    def k_launch(e, a, kind, K, n):
        key = (id(e), kind, K)
        if key not in slots:
            slots[key] = e.new_step_slots(K, packed=(kind == "packed"))
        if kind == "packed":
            pk, go = e.step_continuous_autoreset(a, n_steps=n, slots=slots[key]) if cont else e.step_autoreset_packed(a, slots[key], n_steps=n)
            return pk[..., :wdt], pk[..., wdt], pk[..., wdt + 1].to(torch.uint8), go
        return e.step_continuous_autoreset(a, n_steps=n, slots=slots[key]) if cont else e.step_autoreset_n(a, n_steps=n, slots=slots[key])

    for launch, (kind, K, n) in enumerate(plan):
        raw, fed = run.draw(K)
        tag = (case.cid, kind, launch)
        if kind == "single":
            a = torch.from_numpy(raw[0]).cuda()
            out = env.step_continuous_autoreset(a) if cont else env.step_autoreset(a)
            assert _form_is(env, (single_form, 0)), (tag, env.last_step_form)
            if twin is not None:
                _same_bits(tag, env, twin, out, twin.step_continuous_autoreset(a) if cont else twin.step_autoreset(a))
            _assert_outputs(tag, *[v.cpu().numpy() for v in out], run.step(fed[0]))
            _assert_state(tag, env, run)
        else:
            a = torch.from_numpy(raw).cuda()
            out = k_launch(env, a, kind, K, n)
            assert _form_is(env, k_form), (tag, env.last_step_form)
            if twin is not None:
                twin_out = k_launch(twin, a, kind, K, n)
                assert twin_form is None or _form_is(twin, twin_form), (tag, twin.last_step_form)
                _same_bits(tag, env, twin, [v[:n] for v in out], [v[:n] for v in twin_out])
            obs, rew, done, go = [v.cpu().numpy() for v in out]
            for t in range(n):
                _assert_outputs(tag + (t,), obs[t], rew[t], done[t], go[t], run.step(fed[t]))
            _assert_state(tag, env, run)
        if after_launch is not None:
            after_launch(launch)


def drive_gpu(case, env, single_form, k_form, start_episode=None, twin=None, twin_form=None, after_launch=None):
    """`env` (configured with case.over, seeded with case.seed, at world_offset case.offset) reset and taken through the case's launches
    beside the oracle: flags, float32 state, is_learning / num_other and the episode counters exact, float64 state <= 1e-9 (<= 1e-12 as
    generated), observations and rewards <= 1e-5 -- after every single step, in every slot of a K-step launch (plain and packed records),
    the state after every launch; every launch asserts the form that ran.  start_episode (uint32 [W]): the env is seeded with these
    per-world episode counters first.  twin, twin_form, after_launch: drive_plan's.  Returns the oracle run (its events: assert_events)."""
    import torch
    run = OracleRun(case, start_episode)
    for e in (env,) if twin is None else (env, twin):
        if start_episode is not None:
            e.seed(case.seed, torch.from_numpy(np.asarray(start_episode, np.uint32).view(np.int32).copy()).to(e.device))
        obs0 = e.reset().cpu().numpy()
        _assert_state((case.cid, "reset"), e, run, GEN_TOL)
        oobs0 = co.observe(run.cfg, run.st)
        assert float(rp.obs_diff(obs0, oobs0).max()) <= OBS_TOL and np.array_equal(obs0[..., :2], oobs0[..., :2].astype(np.float32)), case.cid
    drive_plan(case, env, run, case.plan, single_form, k_form, twin, twin_form, after_launch)
    return run
