"""What the GPU tests share: the env of a given shape, the hand-over of a world state between the oracle and the env, the step comparison
against the float64 oracle with its tolerances, the library's return codes, and the helpers several files took from one another -- the
launch-form reference and subject (tests/test_gpu_launch_forms.py), the look-ahead twins (tests/test_gpu_lookahead_topup.py), the placed
ORCA worlds (tests/test_gpu_orca_regimes.py).  A plain module: no test file imports another, tools/ import from here too, and pytest does
not rewrite its asserts, so each carries its own message."""
import math
import os

import numpy as np
import torch

from tests.cfg_regimes import _goal_seeking_actions          # noqa: F401  (shared with the off-default cases; handed on to the callers)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -4                          # CAVOID_OK, CAVOID_EINVAL, CAVOID_EUNSUPPORTED (include/cavoid.h)
OBS_TOL = 1e-5      # tolerance stated by north_star for float observations / rewards
STATE_TOL = 1e-9    # float64 world state (positions, heading, time) after free-running both sides


def _env(W, N, M=None, seed=0, **over):
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.config import EnvConfig

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = N - 1 if M is None else M
            EnvConfig.__init__(self)
    return BatchedCollisionAvoidanceEnv(W, Cfg(), device="cuda:0", seed=seed, **over)


def _push(env, st):
    env.set_state(torch.from_numpy(st.f64).cuda(), torch.from_numpy(st.f32).cuda(),
                  torch.from_numpy(st.flags.view(np.int32)).cuda())


def _pull(env):
    f64, f32, fl = env.get_state()
    return f64.cpu().numpy(), f32.cpu().numpy(), fl.cpu().numpy().view(np.uint32)


def _compare_step(tag, env_out, ora_out, env, st):
    obs, rew, done, go = [t.cpu().numpy() for t in env_out]
    oobs, orew, odone, ogo = ora_out
    assert np.array_equal(done, odone), (tag, "done")
    assert np.array_equal(go, ogo), (tag, "game_over")
    f64, f32, fl = _pull(env)
    assert np.array_equal(fl, st.flags), (tag, "flags")            # every flag bit, incl. collision / goal
    assert np.array_equal(f32, st.f32), (tag, "f32 state")
    np.testing.assert_allclose(f64, st.f64, rtol=0, atol=STATE_TOL, err_msg=str((tag, "f64 state")))
    np.testing.assert_allclose(rew, orew, rtol=0, atol=OBS_TOL, err_msg=str((tag, "rewards")))
    # heading_ego_frame (col 3) is an ANGLE: the reference's wrap() has its branch cut at +-pi, and an
    # agent that has just run over its goal centre sits exactly on it (goal dead astern), where a
    # 1-ulp atan2 difference turns -pi into +pi.  Compare that column on the circle; all else plain.
    dh = np.abs(obs[..., 3].astype(np.float64) - oobs[..., 3])
    dh = np.minimum(dh, np.abs(dh - 2.0 * np.pi))
    assert dh.max() <= OBS_TOL, (tag, "obs heading", dh.max())
    keep = np.ones(obs.shape[-1], bool)
    keep[3] = False
    np.testing.assert_allclose(obs[..., keep], oobs[..., keep], rtol=0, atol=OBS_TOL, err_msg=str((tag, "obs")))
    assert np.array_equal(obs[..., :2], oobs[..., :2].astype(np.float32)), (tag, "is_learning, num_other")   # exact


# ---- tests/test_gpu_launch_forms.py, tests/test_gpu_relay_duo.py: one reference env beside the launch forms -------------------------
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
F_IN_COLL, F_PRESENT = 0x04, 0x20
ENV_VARS = ("CAVOID_QUAD", "CAVOID_PIPELINE", "CAVOID_RELAY_CONSUMERS", "CAVOID_PREFETCH_POOL", "CAVOID_WPW")


def _make_env(monkeypatch, W, N, M, seed, env_vars, over):
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.config import EnvConfig

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = N - 1 if M is None else M
            EnvConfig.__init__(self)
    for k in ENV_VARS:                                      # cavoid_create reads them: set for this env only
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CAVOID_QUAD", "0")
    for k, v in env_vars.items():
        monkeypatch.setenv(k, v)
    try:
        return BatchedCollisionAvoidanceEnv(W, Cfg(), device="cuda:0", seed=seed, **over)
    finally:
        for k in ENV_VARS:
            monkeypatch.delenv(k, raising=False)


def _actions(rng, T, W, N, num_actions, straight, p_edge=0.03):
    """(raw, clamped) int32 [T, W, N]: mostly straight ahead (goals are reached, worlds restart), some random, and a few
    out-of-range values of every kind in the raw set."""
    a = rng.integers(0, num_actions, size=(T, W, N)).astype(np.int64)
    a[rng.random((T, W, N)) < 0.6] = straight
    edge = rng.random((T, W, N)) < p_edge
    a[edge] = rng.choice(np.array([-1, num_actions, INT32_MIN, INT32_MAX], np.int64), size=int(edge.sum()))
    return a.astype(np.int32), np.clip(a, 0, num_actions - 1).astype(np.int32)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(x, y, tag):
    if torch.equal(_bits(x), _bits(y)):
        return
    if x.dim() >= 3 and x.shape[0] > 1:                     # which step, for the message
        bad = [t for t in range(x.shape[0]) if not torch.equal(_bits(x[t]), _bits(y[t]))]
        raise AssertionError("%s: first differing step %d of %d (%d differ)" % (tag, bad[0], x.shape[0], len(bad)))
    raise AssertionError(str(tag))


class _Reference(object):
    """env_kernel, one step per launch, the host-clamped actions; every step's outputs kept for the launch being checked."""

    def __init__(self, env, kmax):
        W, N, D = env.num_worlds, env.max_agents, env.obs_width
        self.env = env
        self.obs = torch.empty((kmax, W, N, D), dtype=torch.float32, device=env.device)
        self.rew = torch.empty((kmax, W, N), dtype=torch.float32, device=env.device)
        self.done = torch.empty((kmax, W, N), dtype=torch.uint8, device=env.device)
        self.go = torch.empty((kmax, W), dtype=torch.uint8, device=env.device)
        self.coll = torch.zeros((), dtype=torch.bool, device=env.device)
        self.r_coll = float(env.cfg.reward_collision)

    def run(self, acts):
        for t in range(acts.shape[0]):
            o, r, d, g = self.env.step_autoreset(acts[t])
            assert self.env.last_step_form == ("STEP", 0), ("the reference env ran", self.env.last_step_form, "at step", t)
            self.obs[t].copy_(o); self.rew[t].copy_(r); self.done[t].copy_(d); self.go[t].copy_(g)
            # a collision: the flag of an agent whose world runs on, or the collision reward (the clip's floor) when it ended the world
            self.coll |= ((self.env.get_state()[2] & F_IN_COLL) != 0).any() | (r <= self.r_coll).any()


class _Subject(object):
    """One form, one output kind: 'slots' (every step in its slot), 'packed' (every step's packed records), 'last'
    (out_step_stride = 0)."""

    def __init__(self, env, form, kind, expect, kmax):
        self.env, self.form, self.kind, self.expect = env, form, kind, expect
        self.slots = env.new_step_slots(kmax, packed=(kind == "packed")) if kind != "last" else None

    def launch(self, acts):
        if self.kind == "packed":
            self.env.step_autoreset_packed(acts, self.slots)
        else:
            self.env.step_autoreset_n(acts, slots=self.slots)

    def check(self, ref, K, tag):
        e = self.env
        got = e.last_step_form
        want = ("STEP", 0) if K == 1 else self.expect
        assert got == want, (tag, "ran %r, expected %r" % (got, want))
        if self.kind == "slots":
            s = self.slots
            _same_bits(s.obs[:K], ref.obs[:K], (tag, "obs")); _same_bits(s.rewards[:K], ref.rew[:K], (tag, "rewards"))
            _same_bits(s.done[:K], ref.done[:K], (tag, "done")); _same_bits(s.game_over[:K], ref.go[:K], (tag, "game_over"))
        elif self.kind == "packed":
            p, D = self.slots.packed, e.obs_width
            _same_bits(p[:K, ..., :D], ref.obs[:K], (tag, "packed obs")); _same_bits(p[:K, ..., D], ref.rew[:K], (tag, "packed reward"))
            _same_bits(p[:K, ..., D + 1], ref.done[:K].float(), (tag, "packed done"))
            _same_bits(self.slots.game_over[:K], ref.go[:K], (tag, "packed game_over"))
        else:
            _same_bits(e.obs, ref.obs[K - 1], (tag, "obs")); _same_bits(e.rewards, ref.rew[K - 1], (tag, "rewards"))
            _same_bits(e.done, ref.done[K - 1], (tag, "done")); _same_bits(e.game_over, ref.go[K - 1], (tag, "game_over"))
        for name, x, y in zip(("f64", "f32", "flags"), e.get_state(), ref.env.get_state()):
            _same_bits(x, y, (tag, name))
        _same_bits(e.episode, ref.env.episode, (tag, "episode"))


# ---- tests/test_gpu_lookahead_topup.py, tests/test_gpu_relay_duo.py: look-ahead twins -----------------------------------------------
# one-step episodes: the time budget of a fresh agent is max(MAX_TIME_RATIO * straight-line time, dt), so a vanishing ratio leaves
# exactly one step -- every agent runs out at its first step and EVERY world restarts at EVERY step: the boundary of the host's
# `budget >= n_steps` rule and of "the launch reads no record beyond episode-at-entry + n_steps"
ONE_STEP = dict(max_time_ratio=1e-9)


def _plain_cfg(N):
    from rl_collision_avoidance_amd.config import EnvConfig

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            EnvConfig.__init__(self)
    return Cfg()


def _lookahead_env(W, N, seed, lookahead, **over):
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    kw = dict(gen_pool_size=0, **over)
    if lookahead:
        kw["gen_lookahead"] = lookahead
    return BatchedCollisionAvoidanceEnv(W, _plain_cfg(N), device="cuda:0", seed=seed, **kw)


def _same_state(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.get_state(), b.get_state())) and torch.equal(a.episode, b.episode)


def _same_slots(sa, sb, K):
    return all(torch.equal(getattr(sa, n)[:K], getattr(sb, n)[:K]) for n in ("obs", "rewards", "done", "game_over"))


# ---- tests/test_gpu_rollout.py, tests/test_gpu_rollout_limits.py -------------------------------------------------------------------
def _default_device_env(W, N, seed, **over):
    """an env on the default device, as tests/test_gpu_rollout.py makes it"""
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.config import EnvConfig

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            EnvConfig.__init__(self)
    return BatchedCollisionAvoidanceEnv(W, Cfg(), seed=seed, **over)


# ---- tests/test_gpu_orca_regimes.py and its child process: the placed worlds of tests/orca_regimes.py -------------------------------
def _orca_env(group, N, rvo_enabled):
    from tests import orca_regimes as R
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.config import EnvConfig

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = N - 1
            EnvConfig.__init__(self)
    return BatchedCollisionAvoidanceEnv(R.num_worlds(group, N), Cfg(), device="cuda:0", seed=R.SEED, **R.over_of(group, rvo_enabled))


def _orca_push(env, run):
    """the batch as the oracle run started from it, the episode counters back at 0"""
    from tests import orca_regimes as R
    env.seed(R.SEED, torch.zeros(env.num_worlds, dtype=torch.int32, device=env.device))
    st = run.start
    env.set_state(torch.from_numpy(st.f64).cuda(), torch.from_numpy(st.f32).cuda(), torch.from_numpy(st.flags.view(np.int32)).cuda())


# ---- tests/test_gpu_crowd_rvo.py, tools/crowd_rvo_seeds.py ------------------------------------------------------------------------
def _infeasible_first_programmes(st, N, worlds=6):
    """how many running ORCA agents of worlds 0..worlds-1 have a first programme without a solution (oracle/cavoid_oracle.py's own
    orca_lines / _lp_plane on the pre-move state): those agents take the least-penetration programme"""
    from oracle import cavoid_oracle as po
    cfg = po.OracleConfig(max_agents=N, max_other_agents_observed=N - 1)
    count = 0
    for w in range(worlds):
        k = slice(w * N, (w + 1) * N)
        world = po.world_from_arrays(st.f64[:, k], st.f32[:, k], st.flags[k], cfg)
        for hi, host in enumerate(world.agents):
            if host.policy != po.POLICY_RVO or host.is_done:
                continue
            gx, gy = host.goal[0] - host.pos[0], host.goal[1] - host.pos[1]
            gn = math.sqrt(gx * gx + gy * gy)
            scale = host.pref_speed / gn if gn > 0.0 else 0.0
            lines = po.orca_lines(hi, world.agents, cfg)
            fail, _, _ = po._lp_plane(lines, host.pref_speed, scale * gx, scale * gy, False)
            count += fail < len(lines)
    return count
