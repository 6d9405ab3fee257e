"""GPU tests of the crowd worlds' fused actor loop for the weight_sharing network (`cavoid_crowd_actor_run_ws`,
csrc/cavoid_crowd_actor_ws.hpp: `crowd_ws_rollout_kernel<NB, RVO>`): K closed-loop GA3C actor steps of worlds of 17..64 agents -- the
weight_sharing pass on the tile's live rows with the input slots as a ring, the action draw, the crowd env step, the Experience bookkeeping
and the episode log -- in ONE launch, against the same K steps taken one launch at a time (`BatchedRollout.step`: row list,
`policy_ws_forward_kernel` / `policy_wsring_forward_kernel`, `crowd_push_kernel`: the code of before, untouched).  The fused kernel runs the
very same statements per value, so everything must be BIT-identical: observations, world state, episode counters, the experience rings, the
training rows handed to the trainer; only the episode totals are compared to float32 rounding (unordered double atomics).

Worlds must end and restart inside the runs, or the bookkeeping half is compared on nothing: an untrained network does not bring crowd agents
to their goals, so every case but the first and the last sets max_time_ratio = 0.1 -- every agent then times out whatever it is given --
and every case asserts on the step-by-step side that episodes ended, rows were drained and episode records written."""
import pytest

torch = pytest.importorskip("torch")

from tests import actor_twins as tw
from tests.actor_twins import FAST, KS, ORCA, close as _close, compare_twins as _compare
from tests.gpu_support import EINVAL, EUNSUPPORTED, OK

pytestmark = pytest.mark.gpu

ARGS = ["--agents", "20", "--arch", "weight_sharing"]       # the train CLI's shape in this file


def _make(W, N, M, seed, reflush=False, greedy=False, arch="weight_sharing", net_M=None, time_max=5, frozen=False, **over):
    # the whole-row handle up to 19 observed neighbours, the ring handle above (ws_crowd=None); room for every duplicate row of the
    # re-flush quirk: at most one per slot and step
    return tw.make(W, N, M, seed, reflush, greedy, arch=arch, net_M=net_M, ws_crowd=None, frozen="learner" if frozen else False,
                   dup_capacity=W * N * 160, time_max=time_max, **over)


def _run(env, roll, pol, n_steps=2, same_buffer=False):
    return tw.raw_run(tw.CROWD_WS, env, roll, pol, n_steps, same_buffer=same_buffer)


# (N, W, M, settings): the smallest shapes at which the lane mapping, the row list or the ring can go wrong
@pytest.mark.parametrize("N,W,M,over", [
    # WS-8: three worlds per tile, a ragged last tile, M < N - 1, absent and scripted slots; the default time ratio
    (17, 50, 7, dict(sort_method="closest_first", gen_min_agents=2, gen_nonlearning_fraction=0.3)),
    (20, 24, 19, dict(reflush=True, **FAST)),                                  # M = R, every row runs
    (21, 24, 20, dict(**FAST)),                                                # R + 1: the first refill
    (22, 33, 21, dict(gen_mode=1, gen_pool_size=0, **FAST)),                   # two worlds per tile, box scenarios generated in the step
    (33, 20, 32, dict(greedy=True, sort_method="closest_last", **FAST)),  # one world per tile, 31 idle lanes
    (48, 10, 47, dict(**FAST)),                                                # above 2 R: a slot refilled twice
    (64, 12, 63, dict(reflush=True, gen_min_agents=2, gen_nonlearning_fraction=0.2, **FAST)),   # all 64 lanes, three refills of a slot
    (20, 30, 19, dict(**ORCA, **FAST)),                                        # ORCA agents (crowd_ws_rollout_kernel<32, true>)
    (40, 12, 39, dict(**ORCA, **FAST)),                                        # ... <64, true>
    (33, 520, 7, dict(**FAST)),                                                # 520 workgroups: two per CU on every CU
    # the backward pass past its 32 registers (the serial form), rs.require_deep_flushes: the default time ratio as in the first case --
    # episodes must outlast a chunk of 33 rows (with max_time_ratio = 0.1 the step-by-step side came to 15 such chunks, under the bar of 20)
    (20, 32, 7, dict(time_max=33, gen_min_agents=2, gen_nonlearning_fraction=0.3)),
])
def test_fused_crowd_ws_actor_equals_step_by_step(N, W, M, over):
    over = dict(over)
    reflush, greedy = over.pop("reflush", False), over.pop("greedy", False)
    twin_a, twin_b = _make(W, N, M, 21, reflush, greedy, **over), _make(W, N, M, 21, reflush, greedy, **over)
    env_a, _, pol_a, a = twin_a
    assert a.crowd_ws_fused_available, a.crowd_ws_fused_unavailable_reason
    # (the other paths stay what they were)
    assert not a.fused_available and "more than 16 agents" in a.actor_path
    assert not a.crowd_fused_available and "weight_sharing" in a.crowd_fused_unavailable_reason
    assert not a.ws_fused_available and ("ring" if M > 19 else "crowd worlds") in a.ws_fused_unavailable_reason
    assert pol_a.max_others == M == env_a.cfg.max_other
    time_max = over.get("time_max", 5)
    tw.fused_equals_step_by_step(
        tw.CROWD_WS, twin_a, twin_b, ("crowd ws actor", N, W, M, reflush), ks=KS,
        step_form=("CROWD_RVO", 0) if over.get("rvo_enabled") else ("CROWD", 0),
        check_step_side=tw.step_side("crowd ws actor", N, W, M, reflush),
        deep_flushes=(time_max, "crowd ws actor N=%d W=%d reflush=%s" % (N, W, reflush)) if time_max > 5 else None)


@pytest.mark.parametrize("N,W,M", [(20, 24, 7), (33, 20, 32)])
def test_fused_crowd_ws_actor_graph_replay_equals_eager_calls(N, W, M):
    """`capture_fused_crowd_ws`: the K-step launch as a one-node hipGraph; replays advance the device-side counters like eager calls -- one
    more step() on each side lands in the same ring block and draws the same actions only if both counters agree."""
    twin_a, twin_b = _make(W, N, M, 3, **FAST), _make(W, N, M, 3, **FAST)
    tw.graph_replay(tw.CROWD_WS, twin_a, twin_b, 3, _compare, one_more_step=True, refused_steps_per_graph=3)
    _close((twin_a[0], twin_a[3]), (twin_b[0], twin_b[3]))


def test_fused_crowd_ws_actor_refuses_what_it_does_not_carry():
    made = []

    def refused(code, word, *args, **kw):
        env, _, pol, roll = _make(*args, **kw)
        made.append((env, roll))
        return tw.refused(tw.CROWD_WS, env, pol, roll, code, word, reason_in_error=True)
    tile = refused(EUNSUPPORTED, "run_fused_ws", 32, 4, 7, 1)                        # a tile env: cavoid_actor_run_ws carries it
    assert tile.ws_fused_available
    refused(EUNSUPPORTED, "rnn network", 24, 20, 19, 1, arch="rnn")
    refused(EUNSUPPORTED, "holonomic", 24, 20, 7, 1, dynamics=2)
    # an env whose generator makes frozen-network agents (the rollout insists on a frozen_policy for it: the learner's handle serves)
    refused(EUNSUPPORTED, "frozen-network agents", 24, 20, 7, 1, frozen=True, gen_min_agents=2, gen_nonlearning_fraction=0.5, gen_frozen_fraction=0.5)
    refused(EINVAL, "the env's rows carry 7", 24, 20, 7, 1, net_M=3)                 # a handle whose M differs from the env's
    # n_steps = 0: CAVOID_OK, and nothing changes
    env, _, pol, roll = _make(24, 20, 7, 1)
    made.append((env, roll))
    roll.run_fused_crowd_ws(3)
    tensors = lambda: (roll._obs_buffers[0], roll._obs_buffers[1], roll.x, roll.val, roll.ret, roll.act_ring, roll.emit_t, roll.dup_count, roll.ep_count,
                       roll._act_out, roll._val_out, env.episode, env.rewards, env.done, env.game_over, *env.get_state())
    assert tw.unchanged_by(lambda: _run(env, roll, pol, n_steps=0), tensors, "cavoid_crowd_actor_run_ws with n_steps = 0") == OK
    # ... and a same-buffer call is an argument error, as for cavoid_actor_run
    assert tw.unchanged_by(lambda: _run(env, roll, pol, same_buffer=True), tensors, "cavoid_crowd_actor_run_ws with one buffer twice") == EINVAL
    _close(*made)


def test_train_cli_with_the_flag_runs_the_crowd_ws_actor_kernel(tmp_path):
    tw.train_cli_runs_the_kernel(tmp_path, ARGS + ["--fused-crowd-ws-actor"],
                                 "actors: fused crowd weight_sharing actor kernel (cavoid_crowd_actor_run_ws), 4 env steps per launch")


def test_train_cli_without_the_flag_prints_todays_line(tmp_path):
    tw.train_cli_prints_todays_line(
        tmp_path, ARGS,
        "actors: one launch per phase (policy, env + bookkeeping) -- fused kernel not applicable: more than 16 agents per world "
        "(the crowd step form has no fused actor kernel); in a hipGraph, 4 env steps per graph", "cavoid_crowd_actor_run_ws")


def test_train_cli_with_the_flag_ends_where_the_kernel_does_not_apply(tmp_path):
    """with a reason the run ends with SystemExit naming it (in this process: nothing is captured or trained before that)"""
    from rl_collision_avoidance_amd.ga3c import train
    with pytest.raises(SystemExit, match="--fused-crowd-ws-actor.*not a FusedPolicy"):
        train.main(["--agents", "20", "--arch", "weight_sharing", "--worlds", "64", "--episodes", "64", "--pretrain-steps", "0", "--print-every", "0",
                    "--train-rows", "2048", "--checkpoint-dir", str(tmp_path / "ck"), "--fused-crowd-ws-actor", "--torch-policy"])
