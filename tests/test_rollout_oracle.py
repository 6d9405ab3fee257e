"""The rollout oracle (oracle/rollout_oracle.py) is PINNED here: bit-for-bit against golden vectors
produced by the reference's own ProcessAgent (tests/golden/rollout_golden.npz, rollout_seed7_golden.npz)."""
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
