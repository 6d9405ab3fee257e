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
Case = collections.namedtuple("Case", "cid family N W seed over fields plan acts straight expect pipe forms")


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
    return out


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

    def __init__(self, case, **changed):
        self.case = case
        self.cfg, self.gen = oracle_for(case, **changed)
        self.st = co.State.empty(case.W, case.N)
        self.ep = np.zeros(case.W, np.uint32)
        co.generate(self.cfg, self.gen, case.seed, self.st, self.ep)
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
        out = co.step_autoreset(cfg, self.gen, c.seed, st, self.ep, None if c.acts == "cont" else fed, cont=fed if c.acts == "cont" else None)
        obs, rew, done, go = out
        self.t += 1
        s = self.seen
        present = (st.flags.reshape(c.W, c.N) & F_PRESENT) != 0         # (a restarted world: its new episode, as in the observation)
        n_world = present.sum(axis=1, keepdims=True)
        s["restart"] += int(go.sum())
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


# conditions, not measurements: the share of worlds that restarted within a continuous-action case's steps
MIN_RESTART_SHARE = {17: 0.3, 24: 0.3, 33: 0.2, 64: 0.2}


def assert_events(case, run):
    """what the case must have seen by its last step; if a seed or a step count misses one, another is picked -- the condition stays"""
    for ev in case.expect:
        if ev == "restart_share":
            assert run.restart_share() >= MIN_RESTART_SHARE[case.N], (case.cid, ev, run.restart_share())
        elif ev == "every_world_restarts":
            assert run.ep.min() >= 1, (case.cid, ev)
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


def drive_gpu(case, env, single_form, k_form):
    """`env` (configured with case.over, seeded with case.seed) reset and taken through the case's launches beside the oracle: flags,
    float32 state, is_learning / num_other and the episode counters exact, float64 state <= 1e-9 (<= 1e-12 as generated), observations
    and rewards <= 1e-5 -- after every single step, in every slot of a K-step launch (plain and packed records), the state after every
    launch; every launch asserts the form that ran.  Returns the oracle run (its events: assert_events)."""
    import torch
    run = OracleRun(case)
    cont = case.acts == "cont"
    obs0 = env.reset().cpu().numpy()
    _assert_state((case.cid, "reset"), env, run, GEN_TOL)
    oobs0 = co.observe(run.cfg, run.st)
    assert float(rp.obs_diff(obs0, oobs0).max()) <= OBS_TOL and np.array_equal(obs0[..., :2], oobs0[..., :2].astype(np.float32)), case.cid
    wdt = env.obs_width
    slots = {}
    for launch, (kind, K, n) in enumerate(case.plan):
        raw, fed = run.draw(K)
        tag = (case.cid, kind, launch)
        if kind == "single":
            a = torch.from_numpy(raw[0]).cuda()
            out = env.step_continuous_autoreset(a) if cont else env.step_autoreset(a)
            assert env.last_step_form == (single_form, 0), (tag, env.last_step_form)
            _assert_outputs(tag, *[v.cpu().numpy() for v in out], run.step(fed[0]))
            _assert_state(tag, env, run)
            continue
        key = (kind, K)
        if key not in slots:
            slots[key] = env.new_step_slots(K, packed=(kind == "packed"))
        a = torch.from_numpy(raw).cuda()
        if kind == "packed":
            pk, go = env.step_continuous_autoreset(a, n_steps=n, slots=slots[key]) if cont else env.step_autoreset_packed(a, slots[key], n_steps=n)
            obs, rew, done = pk[..., :wdt], pk[..., wdt], pk[..., wdt + 1].to(torch.uint8)
        else:
            obs, rew, done, go = (env.step_continuous_autoreset(a, n_steps=n, slots=slots[key]) if cont
                                  else env.step_autoreset_n(a, n_steps=n, slots=slots[key]))
        assert env.last_step_form == k_form, (tag, env.last_step_form)
        obs, rew, done, go = [v.cpu().numpy() for v in (obs, rew, done, go)]
        for t in range(n):
            _assert_outputs(tag + (t,), obs[t], rew[t], done[t], go[t], run.step(fed[t]))
        _assert_state(tag, env, run)
    return run
