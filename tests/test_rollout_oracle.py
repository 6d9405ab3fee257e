"""The rollout oracle (oracle/rollout_oracle.py) is PINNED here: bit-for-bit against golden vectors
produced by the reference's own ProcessAgent (tests/golden/rollout_golden.npz, rollout_seed7_golden.npz; off the reference's
default TIME_MAX: rollout_limits_golden.npz)."""
import os

import numpy as np
import pytest

from oracle import rollout_oracle as ro

GOLD = os.path.join(os.path.dirname(__file__), "golden", "rollout_golden.npz")
GOLD7 = os.path.join(os.path.dirname(__file__), "golden", "rollout_seed7_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_survey_probe_returns(gold):
    # SURVEY.md section 8c probe: 5 exps, r = 0.1 t, gamma 0.97, bootstrap 0.5
    buf = [ro.Entry(np.zeros(26), 0, 0.1 * t, False) for t in range(5)]
    rows, left = ro.n_step_returns(buf, 0.97, 0.5, False, 20)
    got = np.array([e.reward for e in rows])
    assert left is None and np.array_equal(got, gold["probe_returns"])
    np.testing.assert_allclose(got, [1.001628, 1.032606, 0.96145, 0.785], atol=5e-7)


def test_accumulate_rewards_golden(gold):
    gamma, t_max = float(gold["discount"]), int(gold["time_max"])
    assert (gamma, t_max) == (0.97, 20)
    for k in range(int(gold["acc_n"])):
        g = lambda name: gold["acc_%d_%s" % (k, name)]
        rew, done, terminal = g("rew"), bool(g("done")), float(g("terminal"))
        buf = [ro.Entry(np.full(26, float(j)), j % 11, float(rew[j]), done and j == len(rew) - 1) for j in range(len(rew))]
        rows, left = ro.n_step_returns(buf, gamma, terminal, done, t_max)
        x, r, a = ro.to_arrays(rows, 11)
        assert np.array_equal(r, g("r_out")), k
        assert np.array_equal(x[:, 0].astype(np.int64), g("idx_out")), k
        assert a.dtype == np.float32 and np.array_equal(a, g("a_out")), k
        assert (-1 if left is None else int(left[0].state[0])) == int(g("leftover")), k
        assert np.array_equal(np.array([e.reward for e in buf]), g("rew_after")), k


def _episode(gold, e):
    g = lambda name: gold["ep_%d_%s" % (e, name)]
    return dict(obs=g("obs"), rewards=g("rewards"), done=g("done"), learning=g("learning"), n_present=int(g("n")),
                actions=g("actions"), values=g("values"))


def test_run_episode_golden(gold):
    saw_leftover = saw_reflush = saw_tmax = False
    for e in range(int(gold["num_episodes"])):
        g = lambda name: gold["ep_%d_%s" % (e, name)]
        chunks = ro.run_episode(gamma=0.97, t_max=20, **_episode(gold, e))
        assert len(chunks) == int(g("num_yields")), e
        assert [len(c.r) for c in chunks] == list(g("rows")), e
        D = g("obs").shape[-1] - 1
        x = np.concatenate([c.x.reshape(-1, D) for c in chunks])
        assert np.array_equal(x, g("x")), e
        assert np.array_equal(np.concatenate([c.r for c in chunks]), g("r")), e
        assert np.array_equal(np.concatenate([c.a for c in chunks]), g("a")), e
        assert np.array_equal(np.array([c.score for c in chunks]), g("reward_sum")), e
        saw_leftover |= any(c.leftover for c in chunks)
        saw_tmax |= any(len(c.r) == 20 and not c.leftover for c in chunks)
        per_agent = {}
        for c in chunks:
            per_agent.setdefault(c.agent, []).append(c)
        saw_reflush |= any(sum(1 for c in cs if len(c.r) == 2) >= 3 for cs in per_agent.values())
    assert saw_leftover and saw_reflush and saw_tmax      # the golden set exercises every quirk


def test_against_live_reference():
    """ten more episodes (rng 7) as the reference's run_episode returned them, recorded by
    ``tests/golden/make_rollout_golden.py --seed7`` (tests/golden/rollout_seed7_golden.npz): every yield, bit for bit"""
    g7 = np.load(GOLD7)
    assert (float(g7["discount"]), int(g7["time_max"])) == (0.97, 20)
    for e in range(int(g7["num_episodes"])):
        g = lambda name: g7["ep_%d_%s" % (e, name)]
        mine = ro.run_episode(g("obs"), g("rewards"), g("done"), g("learning"), int(g("n")), g("actions"), g("values"), 0.97, 20)
        assert len(mine) == int(g("num_yields")), e
        for k, c in enumerate(mine):
            assert np.array_equal(g("y%d_x" % k), c.x) and np.array_equal(g("y%d_r" % k), c.r), (e, k)
            assert np.array_equal(g("y%d_a" % k), c.a) and float(g("y%d_score" % k)) == c.score, (e, k)


GOLD_LIMITS = os.path.join(os.path.dirname(__file__), "golden", "rollout_limits_golden.npz")
LIMIT_CASES = ((1, 0.97), (2, 0.97), (31, 0.97), (32, 0.97), (33, 1.0), (40, 0.97))


def _same_yields(mine, rows, x, r, a, score, where):
    """every yield of the reference against the oracle's chunks, bit for bit: count, rows per yield, x, r, a, score"""
    assert len(mine) == len(rows), where
    assert [len(c.r) for c in mine] == list(rows), where
    D = x.shape[1]
    assert np.array_equal(np.concatenate([c.x.reshape(-1, D) for c in mine]), x), where
    assert np.array_equal(np.concatenate([c.r for c in mine]), r), where
    got_a = np.concatenate([c.a for c in mine])
    assert got_a.dtype == np.float32 and np.array_equal(got_a, a), where
    assert np.array_equal(np.array([c.score for c in mine]), score), where


@pytest.mark.parametrize("case", range(len(LIMIT_CASES)), ids=["tmax%d_g%g" % c for c in LIMIT_CASES])
def test_run_episode_limits_golden(case):
    """the oracle off the reference's default TIME_MAX: the reference's own yields at TIME_MAX 1, 2, 31, 32, 33 (undiscounted) and
    40, recorded by ``tests/golden/make_rollout_golden.py --limits`` (tests/golden/rollout_limits_golden.npz)"""
    gl = np.load(GOLD_LIMITS)
    assert tuple(map(tuple, gl["cases"])) == LIMIT_CASES
    t_max, gamma = LIMIT_CASES[case]
    longest = 0
    for e in range(int(gl["num_episodes"])):
        g = lambda name: gl["c%d_ep_%d_%s" % (case, e, name)]
        mine = ro.run_episode(g("obs"), g("rewards"), g("done"), g("learning"), int(g("n")), g("actions"), g("values"), gamma, t_max)
        _same_yields(mine, g("rows"), g("x"), g("r"), g("a"), g("score"), (t_max, e))
        longest = max(longest, int(g("rows").max()))
    assert longest == t_max           # a full time-max flush happened: the case is about ITS buffer length


@pytest.mark.parametrize("t_max,gamma", LIMIT_CASES + ((254, 0.97),), ids=lambda v: "%g" % v)
def test_limits_against_live_reference(t_max, gamma):
    """the same cases, and TIME_MAX = 254 (the largest the library accepts; too long for a fixture), against the reference's
    ProcessAgent itself where it is installed"""
    if not os.path.isdir("/root/reference/ga3c/GA3C"):
        pytest.skip("the reference is not on this machine")
    import importlib.util
    import sys
    saved_path, saved_modules = list(sys.path), set(sys.modules)
    saved_env = {k: os.environ.get(k) for k in ("GYM_CONFIG_CLASS", "GYM_CONFIG_PATH")}
    try:
        spec = importlib.util.spec_from_file_location("_make_rollout_golden", os.path.join(os.path.dirname(GOLD), "make_rollout_golden.py"))
        maker = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(maker)
        assert maker.LIMIT_CASES == LIMIT_CASES
        results = maker.run_limit_case(t_max, gamma, n_episodes=3 if t_max == 254 else maker.LIMIT_EPISODES)
    finally:                          # the maker puts the reference on sys.path: no other test may see it
        sys.path[:] = saved_path
        for m in set(sys.modules) - saved_modules:
            del sys.modules[m]
        for k, v in saved_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    longest = 0
    for e, (s, ys) in enumerate(results):
        mine = ro.run_episode(s["obs"], s["rewards"], s["done"], s["learning"], s["n"], s["actions"], s["values"], gamma, t_max)
        _same_yields(mine, [len(y[1]) for y in ys], np.concatenate([y[0].reshape(-1, 26) for y in ys]), np.concatenate([y[1] for y in ys]),
                     np.concatenate([y[2] for y in ys]), np.array([y[3] for y in ys]), (t_max, e))
        longest = max(longest, max(len(y[1]) for y in ys))
    assert longest == t_max
