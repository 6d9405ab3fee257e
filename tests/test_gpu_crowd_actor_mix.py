"""GPU tests of the crowd worlds' fused actor loop with frozen-network agents (`cavoid_crowd_actor_run_mix`, csrc/cavoid_crowd_actor_mix.hpp:
`crowd_mix_rollout_kernel<NB, RVO>`): K closed-loop GA3C actor steps of worlds of 17..64 agents -- the ring form of the policy pass, the same
pass once more on a second, frozen network for the tile's running frozen-network agents (scripted policy 4), the action draw, the crowd env
step, the Experience bookkeeping and the episode log -- in ONE launch, against the same K steps taken one launch at a time
(`BatchedRollout.step`: row lists, `cavoid_policy_forward[_rows]` on both handles, `crowd_push_kernel`: the code of before, untouched).  The
fused kernel runs the very same statements per value, so everything must be BIT-identical; only the episode totals are compared to float32
rounding (unordered double atomics), as in tests/test_gpu_crowd_actor.py, whose twin construction and comparison this file uses.

Every case sets max_time_ratio = 0.1, so that worlds end and restart inside the run, and asserts on the step-by-step side that a running
frozen-network row was listed at some step, that episodes ended, rows were drained and episode records written: nothing passes on nothing."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_gpu_crowd_actor import FAST, KS, _compare, _make, _same

pytestmark = pytest.mark.gpu

MIX = dict(gen_nonlearning_fraction=0.5, gen_frozen_fraction=0.5)            # (with the default static share: about a quarter frozen-network agents)
# ORCA agents AND frozen-network agents: the settings of tests/test_gpu_crowd_ws_eval.py (the default static share leaves no room for them)
ORCA_MIX = dict(rvo_enabled=2, gen_rvo_fraction=0.5, gen_static_fraction=0.1, gen_frozen_fraction=0.3, gen_nonlearning_fraction=0.5)


def _frozen_rows_spy(env):
    """counts, per step() of the step-by-step twin, the running frozen-network rows it listed"""
    from rl_collision_avoidance_amd import _lib
    counts, rows_of = [], env.policy_rows

    def spy(policy_id, only_running=True):
        out = rows_of(policy_id, only_running)
        if policy_id == _lib.POLICY_FROZEN_NET:
            counts.append(out[1].clone())
        return out
    env.policy_rows = spy
    return counts


# (N, W, M, reflush, greedy, settings): the smallest shapes at which the lane mapping, the ring or the second pass can go wrong
@pytest.mark.parametrize("N,W,M,reflush,greedy,over", [
    (17, 50, 16, False, False, dict(gen_min_agents=2, **MIX)),                 # three worlds per tile, a ragged last tile, absent slots, no ring refill
    (20, 24, 19, True, False, dict(**MIX)),                                    # every learner row runs: the frozen rows' actions are overwritten after the learner's emit
    (25, 21, 24, False, False, dict(**MIX)),                                   # the first ring refill, on both handles
    (33, 20, 32, False, True, dict(**MIX)),                                    # one world per tile; greedy
    (33, 20, 19, False, False, dict(**MIX)),                                   # M < N - 1
    (48, 10, 47, False, False, dict(**MIX)),                                   # a ring slot refilled twice
    (64, 12, 63, False, False, dict(**MIX)),                                   # all 64 lanes
    (20, 30, 19, False, False, dict(**ORCA_MIX)),                              # ORCA + frozen (crowd_mix_rollout_kernel<32, true>)
    (40, 12, 39, False, False, dict(**ORCA_MIX)),                              # ... <64, true>
    (33, 520, 32, False, False, dict(**MIX)),                                  # 520 workgroups: two per CU on every CU
])
def test_fused_crowd_mix_actor_equals_step_by_step(N, W, M, reflush, greedy, over):
    seed = 21
    env_a, net_a, pol_a, a = _make(W, N, M, seed, reflush, greedy, frozen=True, **FAST, **over)
    env_b, net_b, pol_b, b = _make(W, N, M, seed, reflush, greedy, frozen=True, **FAST, **over)
    assert a.crowd_mix_fused_available, a.crowd_mix_fused_unavailable_reason
    assert not a.fused_available and not a.crowd_fused_available                 # (the existing switches say what they said)
    assert "frozen-network agents" in a.crowd_fused_unavailable_reason
    assert pol_a.max_others == M == env_a.cfg.max_other == a.frozen_policy.max_others
    for p, q in zip(net_a.parameters(), net_b.parameters()):
        assert torch.equal(p, q)
    _same(a.obs, b.obs, "first observation")
    listed = _frozen_rows_spy(env_b)
    form = ("CROWD_RVO", 0) if over.get("rvo_enabled") else ("CROWD", 0)
    total = 0
    for k in KS:
        a.run_fused_crowd_mix(k)
        for _ in range(k):
            b.step()
        total += k
        _compare(env_a, a, env_b, b, total)
        assert env_a.last_step_form == form and env_b.last_step_form == form
    # the step-by-step side (the code of before) did what the case is about: nothing below passes on nothing
    frozen_seen = torch.stack(listed).view(-1).cpu().numpy()
    dup_b = b.dup_count.tolist()
    ba, bb = a.drain(flush_all=True), b.drain(flush_all=True)
    ea, eb = a.drain_episodes().cpu().numpy(), b.drain_episodes().cpu().numpy()
    print("crowd mix actor N=%d W=%d M=%d: step-by-step side: frozen rows listed at %d of %d steps (max %d), episode max %d, drained %d rows, "
          "%d duplicates (%d dropped), %d episode records" % (N, W, M, int((frozen_seen > 0).sum()), len(frozen_seen), int(frozen_seen.max()),
                                                              env_b.episode.max().item(), len(bb), dup_b[0], dup_b[1], len(eb)))
    assert len(frozen_seen) == total and int(frozen_seen.max()) >= 1
    assert env_b.episode.max().item() >= 1
    assert len(bb) > 0 and len(eb) > 0
    assert dup_b[1] == 0 and (dup_b[0] > 0 if reflush else dup_b[0] == 0)
    # what reaches the trainer and the stats process
    assert len(ba) == len(bb) and ba.dropped == bb.dropped == 0
    ka = np.lexsort(ba.src.cpu().numpy().T[::-1])
    kb = np.lexsort(bb.src.cpu().numpy().T[::-1])
    for name in ("src", "x", "r", "a_index"):
        assert np.array_equal(getattr(ba, name).cpu().numpy()[ka], getattr(bb, name).cpu().numpy()[kb]), name
    assert len(ea) == len(eb)
    ea, eb = ea[np.lexsort(ea.T[::-1])], eb[np.lexsort(eb.T[::-1])]
    assert np.array_equal(ea[:, 0], eb[:, 0]) and np.array_equal(ea[:, 2], eb[:, 2])
    np.testing.assert_allclose(ea[:, 1], eb[:, 1], rtol=1e-6, atol=1e-6)         # (double atomics whose order varies)
    # and the two forms interleave: each continues where the other stopped
    a.step(); a.run_fused_crowd_mix(3)
    b.run_fused_crowd_mix(2); b.step(); b.step()
    _same(a.obs, b.obs, "interleaved obs")
    for x, y in zip(env_a.get_state(), env_b.get_state()):
        _same(x, y, "interleaved state")
    for name in ("x", "val", "ret", "act_ring", "emit_t"):
        _same(getattr(a, name), getattr(b, name), ("interleaved", name))
    for r in (a, b):
        r.close()
    for e in (env_a, env_b):
        e.close()


def test_without_frozen_agents_the_mix_launch_equals_the_one_network_launch():
    """gen_frozen_fraction = 0 with a frozen_policy given: the second pass never runs, and the launch equals run_fused_crowd of the same seed
    bit for bit (the one-network rollout has no frozen_policy: run_fused_crowd refuses one)"""
    N, W, M = 20, 24, 19
    over = dict(gen_nonlearning_fraction=0.5, gen_frozen_fraction=0.0, **FAST)
    env_a, _, _, a = _make(W, N, M, 21, False, frozen=True, **over)
    env_b, _, _, b = _make(W, N, M, 21, False, frozen=False, **over)
    assert a.crowd_mix_fused_available and b.crowd_fused_available and not b.crowd_mix_fused_available
    assert "no frozen_policy" in b.crowd_mix_fused_unavailable_reason and "run_fused_crowd" in b.crowd_mix_fused_unavailable_reason
    total = 0
    for k in KS[:6]:
        a.run_fused_crowd_mix(k)
        b.run_fused_crowd(k)
        total += k
        _compare(env_a, a, env_b, b, total)
        _same(a._act_out, b._act_out, ("actions", total))
        _same(a._val_out, b._val_out, ("values", total))
    assert env_b.episode.max().item() >= 1 and (b.emit_t >= 0).any()
    for r in (a, b):
        r.close()
    env_a.close(); env_b.close()


@pytest.mark.parametrize("N,W,M", [(20, 24, 19), (33, 20, 32)])
def test_fused_crowd_mix_graph_replay_equals_step_by_step(N, W, M):
    """`capture_fused_crowd_mix(4)`: the K-step launch as a one-node hipGraph against step(); replays advance the device-side counters like
    eager calls -- one more step() on each side lands in the same ring block and draws the same actions only if both counters agree."""
    env_a, _, _, a = _make(W, N, M, 3, False, frozen=True, **FAST, **MIX)
    env_b, _, _, b = _make(W, N, M, 3, False, frozen=True, **FAST, **MIX)
    listed = _frozen_rows_spy(env_b)
    a.capture_fused_crowd_mix(steps_per_graph=4)      # (runs 2 warm-up steps outside the capture)
    a.replay(3)
    for _ in range(14):
        b.step()
    _compare(env_a, a, env_b, b, 14)
    a.step(); b.step()
    _compare(env_a, a, env_b, b, 15)
    assert (a.emit_t >= 0).any() and int(torch.stack(listed).max()) >= 1
    with pytest.raises(ValueError):
        a.capture_fused_crowd_mix(steps_per_graph=3)
    for r in (a, b):
        r.close()
    env_a.close(); env_b.close()


def _run(env, roll, pol, fz, n_steps=2):
    from rl_collision_avoidance_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr())
    b = roll._actor_buffers()
    rc = _lib.lib().cavoid_crowd_actor_run_mix(env._h, pol._h, fz._h if fz is not None else None, roll._h, C.byref(b), p(roll._obs_buffers[0]),
                                               p(roll._obs_buffers[1]), p(env.rewards), p(env.done), p(env.game_over), p(roll._act_out),
                                               p(roll._val_out), n_steps, 0, None)
    torch.cuda.synchronize()
    return rc


def test_fused_crowd_mix_actor_refuses_what_it_does_not_carry():
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    OK, EINVAL, EUNSUPPORTED = 0, -1, -4
    made = []

    def refused(code, word, env, pol, roll, fz):
        made.append((env, roll))
        assert word in roll.crowd_mix_fused_unavailable_reason, roll.crowd_mix_fused_unavailable_reason
        assert not roll.crowd_mix_fused_available
        with pytest.raises(RuntimeError, match="run_fused_crowd_mix does not apply"):
            roll.run_fused_crowd_mix(2)
        state = [t.clone() for t in env.get_state()]
        assert _run(env, roll, pol, fz) == code                  # straight at the C ABI: a code, not a crash
        assert all(torch.equal(u, v) for u, v in zip(state, env.get_state()))

    env, _, pol, roll = _make(32, 4, 3, 1, False, frozen=True, **MIX)                # a tile env: cavoid_actor_run_mix carries it
    refused(EUNSUPPORTED, "cavoid_actor_run_mix", env, pol, roll, roll.frozen_policy)
    assert roll.fused_available
    env, _, pol, roll = _make(24, 20, 7, 1, False, arch="weight_sharing", frozen=True)   # a weight_sharing policy
    refused(EUNSUPPORTED, "weight_sharing", env, pol, roll, roll.frozen_policy)
    env, _, pol, roll = _make(24, 20, 19, 1, False, frozen=True, dynamics=2)
    refused(EUNSUPPORTED, "holonomic", env, pol, roll, roll.frozen_policy)
    env, _, pol, roll = _make(24, 20, 19, 1, False, frozen=False, gen_nonlearning_fraction=0.5)   # no frozen_policy: EINVAL at the C ABI
    refused(EINVAL, "no frozen_policy", env, pol, roll, None)
    assert "run_fused_crowd" in roll.crowd_mix_fused_unavailable_reason

    def with_frozen(fz_net_cfg, arch="rnn"):
        env, _, pol, roll = _make(24, 20, 19, 1, False, frozen=True, **MIX)
        torch.manual_seed(4321)
        fz = FusedPolicy(NetworkVP_rnn(fz_net_cfg(env), arch=arch).to("cuda:0"), seed=0)
        roll.frozen_policy.close()
        roll.frozen_policy = fz                              # (the rollout reads it where it acts: nothing acts here)
        return env, pol, roll, fz

    def narrow_cfg(env):
        from rl_collision_avoidance_amd.config import EnvConfig

        class Cfg(EnvConfig):
            def __init__(self):
                self.MAX_NUM_AGENTS_IN_ENVIRONMENT = 20
                self.MAX_NUM_OTHER_AGENTS_OBSERVED = 10
                EnvConfig.__init__(self)
        return Cfg()
    env, pol, roll, fz = with_frozen(lambda env: env.config, arch="weight_sharing")  # a weight_sharing frozen policy
    refused(EUNSUPPORTED, "frozen policy is the weight_sharing network", env, pol, roll, fz)
    env, pol, roll, fz = with_frozen(narrow_cfg)                                      # a frozen policy of fewer neighbours
    refused(EUNSUPPORTED, "frozen policy observes 10 neighbours", env, pol, roll, fz)
    # n_steps = 0: CAVOID_OK, and nothing changes; null arguments are refused before it is looked at
    env, _, pol, roll = _make(24, 20, 19, 1, False, frozen=True, **MIX)
    made.append((env, roll))
    roll.run_fused_crowd_mix(3)
    before = [t.clone() for t in (roll._obs_buffers[0], roll._obs_buffers[1], roll.x, roll.emit_t, env.episode, env.rewards, *env.get_state())]
    assert _run(env, roll, pol, roll.frozen_policy, n_steps=0) == OK
    assert _run(env, roll, pol, None, n_steps=0) == EINVAL
    after = [roll._obs_buffers[0], roll._obs_buffers[1], roll.x, roll.emit_t, env.episode, env.rewards, *env.get_state()]
    assert all(torch.equal(u, v) for u, v in zip(before, after))
    for e, r in made:
        r.close(); e.close()
