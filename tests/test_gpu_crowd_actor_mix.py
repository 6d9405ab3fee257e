"""GPU tests of the crowd worlds' fused actor loop with frozen-network agents (`cavoid_crowd_actor_run_mix`, csrc/cavoid_crowd_actor_mix.hpp:
`crowd_mix_rollout_kernel<NB, RVO>`): K closed-loop GA3C actor steps of worlds of 17..64 agents -- the ring form of the policy pass, the same
pass once more on a second, frozen network for the tile's running frozen-network agents (scripted policy 4), the action draw, the crowd env
step, the Experience bookkeeping and the episode log -- in ONE launch, against the same K steps taken one launch at a time
(`BatchedRollout.step`: row lists, `cavoid_policy_forward[_rows]` on both handles, `crowd_push_kernel`: the code of before, untouched).  The
fused kernel runs the very same statements per value, so everything must be BIT-identical; only the episode totals are compared to float32
rounding (unordered double atomics), as in tests/test_gpu_crowd_actor.py, whose twin construction and comparison this file uses.

Every case sets max_time_ratio = 0.1, so that worlds end and restart inside the run, and asserts on the step-by-step side that a running
frozen-network row was listed at some step, that episodes ended, rows were drained and episode records written: nothing passes on nothing."""
import pytest

torch = pytest.importorskip("torch")

from tests import actor_twins as tw
from tests.actor_twins import FAST, KS, compare_twins as _compare, same as _same
from tests.gpu_support import EINVAL, EUNSUPPORTED, OK

pytestmark = pytest.mark.gpu


def _make(W, N, M, seed, reflush, greedy=False, net_M=None, arch="rnn", frozen=False, time_max=5, **over):
    # tests/test_gpu_crowd_actor.py's twin: room for every duplicate row of the re-flush quirk, at most one per slot and step
    return tw.make(W, N, M, seed, reflush, greedy, arch=arch, net_M=net_M, ws_crowd=False, frozen="rnn" if frozen else False,
                   dup_capacity=W * N * 160, time_max=time_max, **over)

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
    twin_a = _make(W, N, M, 21, reflush, greedy, frozen=True, **FAST, **over)
    twin_b = _make(W, N, M, 21, reflush, greedy, frozen=True, **FAST, **over)
    env_a, _, pol_a, a = twin_a
    assert a.crowd_mix_fused_available, a.crowd_mix_fused_unavailable_reason
    assert not a.fused_available and not a.crowd_fused_available                 # (the existing switches say what they said)
    assert "frozen-network agents" in a.crowd_fused_unavailable_reason
    assert pol_a.max_others == M == env_a.cfg.max_other == a.frozen_policy.max_others
    listed = _frozen_rows_spy(twin_b[0])

    def frozen_rows_listed(total):                           # the step-by-step side listed a running frozen-network row at some step
        frozen_seen = torch.stack(listed).view(-1).cpu().numpy()
        assert len(frozen_seen) == total and int(frozen_seen.max()) >= 1
        return "frozen rows listed at %d of %d steps (max %d), " % (int((frozen_seen > 0).sum()), len(frozen_seen), int(frozen_seen.max()))
    tw.fused_equals_step_by_step(
        tw.CROWD_MIX, twin_a, twin_b, ("crowd mix actor", N, W, M, reflush), ks=KS,
        step_form=("CROWD_RVO", 0) if over.get("rvo_enabled") else ("CROWD", 0),
        check_step_side=tw.step_side("crowd mix actor", N, W, M, reflush, extra=frozen_rows_listed))


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
    twin_a, twin_b = _make(W, N, M, 3, False, frozen=True, **FAST, **MIX), _make(W, N, M, 3, False, frozen=True, **FAST, **MIX)
    listed = _frozen_rows_spy(twin_b[0])
    tw.graph_replay(tw.CROWD_MIX, twin_a, twin_b, 3, _compare, eager=False, one_more_step=True, refused_steps_per_graph=3)
    assert int(torch.stack(listed).max()) >= 1
    tw.close((twin_a[0], twin_a[3]), (twin_b[0], twin_b[3]))


def _run(env, roll, pol, fz, n_steps=2):
    return tw.raw_run(tw.CROWD_MIX, env, roll, pol, n_steps, fz=fz, cur=0)


def test_fused_crowd_mix_actor_refuses_what_it_does_not_carry():
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    made = []

    def refused(code, word, env, pol, roll, fz):
        made.append((env, roll))
        tw.refused(tw.CROWD_MIX, env, pol, roll, code, word, fz=fz, cur=0, error_match="run_fused_crowd_mix does not apply", state_untouched=True)

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
    tensors = lambda: (roll._obs_buffers[0], roll._obs_buffers[1], roll.x, roll.emit_t, env.episode, env.rewards, *env.get_state())
    codes = tw.unchanged_by(lambda: (_run(env, roll, pol, roll.frozen_policy, n_steps=0), _run(env, roll, pol, None, n_steps=0)), tensors,
                            "cavoid_crowd_actor_run_mix with n_steps = 0")
    assert codes == (OK, EINVAL)
    tw.close(*made)
