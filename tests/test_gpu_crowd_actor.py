"""GPU tests of the crowd worlds' fused actor loop (`cavoid_crowd_actor_run`, csrc/cavoid_crowd_actor.hpp: `crowd_actor_kernel<NB, RVO>`): K
closed-loop GA3C actor steps of worlds of 17..64 agents -- the ring form of the policy pass, the action draw, the crowd env step, the
Experience bookkeeping and the episode log -- in ONE launch, against the same K steps taken one launch at a time (`BatchedRollout.step`: row
list, `policy_crowd_forward_kernel` / `policy_forward_split_kernel`, `crowd_push_kernel`: the code of before, untouched).  The fused kernel
runs the very same statements per value, so everything must be BIT-identical: observations, world state, episode counters, the experience
rings, the training rows handed to the trainer; only the episode totals are compared to float32 rounding (unordered double atomics).

Worlds must end and restart inside the runs, or the bookkeeping half is compared on nothing: an untrained network does not bring crowd agents
to their goals, so every case but the first sets max_time_ratio = 0.1 -- every agent then times out whatever it is given (time-outs do not
depend on actions, collisions only end agents sooner) -- and every case asserts on the step-by-step side that episodes ended, rows were
drained and episode records written."""
import pytest

torch = pytest.importorskip("torch")

from tests import actor_twins as tw
from tests.actor_twins import FAST, KS, ORCA, compare_twins as _compare
from tests.gpu_support import EINVAL, EUNSUPPORTED, OK

pytestmark = pytest.mark.gpu

ARGS = ["--agents", "20"]                                   # the train CLI's shape in this file


def _make(W, N, M, seed, reflush, greedy=False, net_M=None, arch="rnn", frozen=False, time_max=5, **over):
    # room for every duplicate row of the re-flush quirk: at most one per slot and step
    return tw.make(W, N, M, seed, reflush, greedy, arch=arch, net_M=net_M, ws_crowd=False, frozen="rnn" if frozen else False,
                   dup_capacity=W * N * 160, time_max=time_max, **over)


def _run(env, roll, pol, n_steps=2, same_buffer=False):
    return tw.raw_run(tw.CROWD, env, roll, pol, n_steps, cur=0, same_buffer=same_buffer)


# (N, W, M, reflush, greedy, settings): the smallest shapes at which the lane mapping or the ring can go wrong
@pytest.mark.parametrize("N,W,M,reflush,greedy,over", [
    # three worlds per tile, 13 idle lanes, a ragged last tile, an ordinary policy handle (M <= 19); the default time ratio
    (17, 50, 16, False, False, dict(gen_min_agents=2, gen_nonlearning_fraction=0.3)),
    (20, 24, 19, True, False, dict(**FAST)),                                   # the M = 19 boundary; every row runs
    (22, 33, 21, False, False, dict(gen_mode=1, gen_pool_size=0, **FAST)),     # two worlds per tile, box scenarios generated in the step; M <= R: no refill
    (25, 21, 24, False, False, dict(**FAST)),                                  # R + 1: the first refill
    (33, 20, 32, False, True, dict(**FAST)),                                   # one world per tile, 31 idle lanes; greedy
    (33, 20, 19, False, False, dict(**FAST)),                                  # M < N - 1
    (48, 10, 47, False, False, dict(**FAST)),                                  # above 2 R: a slot refilled twice
    (64, 12, 63, True, False, dict(gen_min_agents=2, gen_nonlearning_fraction=0.2, **FAST)),   # all 64 lanes, the full-width world mask
    (20, 30, 19, False, False, dict(**ORCA, **FAST)),                          # ORCA agents (crowd_actor_kernel<32, true>)
    (40, 12, 39, False, False, dict(**ORCA, **FAST)),                          # ... <64, true>
    (33, 520, 32, False, False, dict(**FAST)),                                 # 520 workgroups: two per CU on every CU
    # the backward pass past its 32 registers (the serial form) and with all 32 live; the default time ratio: episodes outlast a chunk
    (20, 32, 19, False, False, dict(time_max=33, gen_min_agents=2, gen_nonlearning_fraction=0.3)),
    (20, 32, 19, True, False, dict(time_max=33, gen_min_agents=2, gen_nonlearning_fraction=0.3)),
    (20, 32, 19, False, False, dict(time_max=31, gen_min_agents=2, gen_nonlearning_fraction=0.3)),
])
def test_fused_crowd_actor_equals_step_by_step(N, W, M, reflush, greedy, over):
    twin_a, twin_b = _make(W, N, M, 21, reflush, greedy, **over), _make(W, N, M, 21, reflush, greedy, **over)
    env_a, _, pol_a, a = twin_a
    assert a.crowd_fused_available, a.crowd_fused_unavailable_reason
    assert not a.fused_available and "more than 16 agents" in a.actor_path       # (the default paths stay what they were)
    assert pol_a.max_others == M == env_a.cfg.max_other
    time_max = over.get("time_max", 5)
    tw.fused_equals_step_by_step(
        tw.CROWD, twin_a, twin_b, ("crowd actor", N, W, M, reflush), ks=KS,
        step_form=("CROWD_RVO", 0) if over.get("rvo_enabled") else ("CROWD", 0),
        check_step_side=tw.step_side("crowd actor", N, W, M, reflush),
        deep_flushes=(time_max, "crowd actor N=%d W=%d reflush=%s" % (N, W, reflush)) if time_max > 5 else None)


@pytest.mark.parametrize("N,W,M", [(20, 24, 19), (33, 20, 32)])
def test_fused_crowd_actor_graph_replay_equals_eager_calls(N, W, M):
    """`capture_fused_crowd`: the K-step launch as a one-node hipGraph; replays advance the device-side counters like eager calls -- one more
    step() on each side lands in the same ring block and draws the same actions only if both counters agree."""
    twin_a, twin_b = _make(W, N, M, 3, False, **FAST), _make(W, N, M, 3, False, **FAST)
    tw.graph_replay(tw.CROWD, twin_a, twin_b, 3, _compare, one_more_step=True, refused_steps_per_graph=3)
    tw.close((twin_a[0], twin_a[3]), (twin_b[0], twin_b[3]))


def test_fused_crowd_actor_refuses_what_it_does_not_carry(monkeypatch):
    made = []

    def refused(code, word, *args, **kw):
        env, _, pol, roll = _make(*args, **kw)
        made.append((env, roll))
        return tw.refused(tw.CROWD, env, pol, roll, code, word, cur=0)
    tile = refused(EUNSUPPORTED, "run_fused", 32, 4, 3, 1, False)                    # a tile env: cavoid_actor_run carries it
    assert tile.fused_available
    crowd = []
    crowd.append(refused(EUNSUPPORTED, "weight_sharing", 24, 20, 7, 1, False, arch="weight_sharing"))
    crowd.append(refused(EUNSUPPORTED, "holonomic", 24, 20, 19, 1, False, dynamics=2))
    crowd.append(refused(EUNSUPPORTED, "frozen-network agents", 24, 20, 19, 1, False, frozen=True, gen_min_agents=2, gen_nonlearning_fraction=0.5,
                         gen_frozen_fraction=0.5))
    crowd.append(refused(EINVAL, "neighbours", 24, 20, 19, 1, False, net_M=10))       # a handle whose M differs from the env's
    monkeypatch.setenv("CAVOID_POLICY_PRODUCTS", "3")                                # (read at handle creation)
    crowd.append(refused(EUNSUPPORTED, "non-default inference form", 24, 20, 19, 1, False))
    monkeypatch.delenv("CAVOID_POLICY_PRODUCTS")
    for roll in crowd:
        assert not roll.fused_available                      # (and the tile forms' kernel is still not theirs)
    # n_steps = 0: CAVOID_OK, and nothing changes
    env, _, pol, roll = _make(24, 20, 19, 1, False)
    made.append((env, roll))
    roll.run_fused_crowd(3)
    tensors = lambda: (roll._obs_buffers[0], roll._obs_buffers[1], roll.x, roll.emit_t, env.episode, env.rewards, *env.get_state())
    assert tw.unchanged_by(lambda: _run(env, roll, pol, n_steps=0), tensors, "cavoid_crowd_actor_run with n_steps = 0") == OK
    # ... and a same-buffer call is an argument error, as for cavoid_actor_run
    assert _run(env, roll, pol, same_buffer=True) == EINVAL
    tw.close(*made)


def test_train_cli_with_the_flag_runs_the_crowd_actor_kernel(tmp_path):
    tw.train_cli_runs_the_kernel(tmp_path, ARGS + ["--fused-crowd-actor"],
                                 "actors: fused crowd actor kernel (cavoid_crowd_actor_run), 4 env steps per launch")


def test_train_cli_without_the_flag_prints_todays_line(tmp_path):
    tw.train_cli_prints_todays_line(
        tmp_path, ARGS,
        "actors: one launch per phase (policy, env + bookkeeping) -- fused kernel not applicable: more than 16 agents per world "
        "(the crowd step form has no fused actor kernel); in a hipGraph, 4 env steps per graph", "cavoid_crowd_actor_run")


def test_train_cli_with_the_flag_ends_where_the_kernel_does_not_apply(tmp_path):
    """with a reason the run ends with SystemExit naming it (in this process: nothing is captured or trained before that)"""
    from rl_collision_avoidance_amd.ga3c import train
    with pytest.raises(SystemExit, match="--fused-crowd-actor.*not a FusedPolicy"):
        train.main(["--agents", "20", "--worlds", "64", "--episodes", "64", "--pretrain-steps", "0", "--print-every", "0", "--train-rows", "2048",
                    "--checkpoint-dir", str(tmp_path / "ck"), "--fused-crowd-actor", "--torch-policy"])
