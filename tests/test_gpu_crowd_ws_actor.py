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
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import rollout_scripts as rs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (2, 1, 7, 16, 4) + (16,) * 7 + (3,)                    # 145 steps; odd counts too: the observation buffers alternate
FAST = dict(max_time_ratio=0.1)
ORCA = dict(rvo_enabled=2, gen_rvo_fraction=0.5, gen_nonlearning_fraction=0.5)
OK, EINVAL, EUNSUPPORTED = 0, -1, -4


def _make(W, N, M, seed, reflush=False, greedy=False, arch="weight_sharing", net_M=None, time_max=5, frozen=False, **over):
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.config import EnvConfig
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import MAX_OTHERS_WS, FusedPolicy
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout

    class Cfg(EnvConfig):
        def __init__(self, m):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = m
            EnvConfig.__init__(self)
    cfg = Cfg(M)
    env = BatchedCollisionAvoidanceEnv(W, cfg, device="cuda:0", seed=seed, **over)
    torch.manual_seed(1234)
    m_net = M if net_M is None else net_M
    net = NetworkVP_rnn(cfg if net_M is None else Cfg(net_M), arch=arch).to("cuda:0")
    # the whole-row handle up to 19 observed neighbours, the ring handle above (ws_crowd=True)
    pol = FusedPolicy(net, seed=77, ws_crowd=(arch == "weight_sharing" and m_net > MAX_OTHERS_WS))
    # skip_finished = not reflush: the fused kernel hands a result only to the rows that still need an action (with the re-flush quirk: to
    # every row), exactly the rows the step-by-step path lists with skip_finished -- like is compared with like.  Room for every duplicate
    # row of the re-flush quirk (at most one per slot and step): a full buffer drops rows in arrival order, which legitimately differs.
    roll = BatchedRollout(env, pol, reflush_done=reflush, greedy=greedy, time_max=time_max, dup_capacity=W * N * 160 if reflush else None,
                          skip_finished=not reflush, frozen_policy=pol if frozen else None)
    roll.reset()
    return env, net, pol, roll


def _same(a, b, what):
    assert torch.equal(a, b), what


def _compare(env_a, a, env_b, b, total):
    _same(a.obs, b.obs, ("obs", total))
    for x, y in zip(env_a.get_state(), env_b.get_state()):
        _same(x, y, ("state", total))
    for name in ("episode", "rewards", "done", "game_over"):
        _same(getattr(env_a, name), getattr(env_b, name), (name, total))
    for name in ("x", "val", "ret", "act_ring", "emit_t", "dup_count"):
        _same(getattr(a, name), getattr(b, name), (name, total))
    assert a.step_index == b.step_index == total


def _close(*pairs):
    for env, roll in pairs:
        roll.close(); env.close()


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
    seed = 21
    env_a, net_a, pol_a, a = _make(W, N, M, seed, reflush, greedy, **over)
    env_b, net_b, pol_b, b = _make(W, N, M, seed, reflush, greedy, **over)
    assert a.crowd_ws_fused_available, a.crowd_ws_fused_unavailable_reason
    # (the other paths stay what they were)
    assert not a.fused_available and "more than 16 agents" in a.actor_path
    assert not a.crowd_fused_available and "weight_sharing" in a.crowd_fused_unavailable_reason
    assert not a.ws_fused_available and ("ring" if M > 19 else "crowd worlds") in a.ws_fused_unavailable_reason
    assert pol_a.max_others == M == env_a.cfg.max_other
    for p, q in zip(net_a.parameters(), net_b.parameters()):
        assert torch.equal(p, q)
    _same(a.obs, b.obs, "first observation")
    form = ("CROWD_RVO", 0) if over.get("rvo_enabled") else ("CROWD", 0)
    total = 0
    for k in KS:
        a.run_fused_crowd_ws(k)
        for _ in range(k):
            b.step()
        total += k
        _compare(env_a, a, env_b, b, total)
        assert env_a.last_step_form == form and env_b.last_step_form == form
    # the step-by-step side (the code of before) did what the case is about: nothing below passes on nothing
    dup_b = b.dup_count.tolist()
    ba, bb = a.drain(flush_all=True), b.drain(flush_all=True)
    ea, eb = a.drain_episodes().cpu().numpy(), b.drain_episodes().cpu().numpy()
    print("crowd ws actor N=%d W=%d M=%d: step-by-step side: episode max %d, drained %d rows, %d duplicates (%d dropped), %d episode records"
          % (N, W, M, env_b.episode.max().item(), len(bb), dup_b[0], dup_b[1], len(eb)))
    assert env_b.episode.max().item() >= 1
    assert len(bb) > 0 and len(eb) > 0
    assert dup_b[1] == 0 and (dup_b[0] > 0 if reflush else dup_b[0] == 0)
    if over.get("time_max", 5) > 5:
        rs.require_deep_flushes(bb.src.cpu().numpy(), over["time_max"], "crowd ws actor N=%d W=%d reflush=%s" % (N, W, reflush))
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
    a.step(); a.run_fused_crowd_ws(3)
    b.run_fused_crowd_ws(2); b.step(); b.step()
    _same(a.obs, b.obs, "interleaved obs")
    for x, y in zip(env_a.get_state(), env_b.get_state()):
        _same(x, y, "interleaved state")
    for name in ("x", "val", "ret", "act_ring", "emit_t"):
        _same(getattr(a, name), getattr(b, name), ("interleaved", name))
    _close((env_a, a), (env_b, b))


@pytest.mark.parametrize("N,W,M", [(20, 24, 7), (33, 20, 32)])
def test_fused_crowd_ws_actor_graph_replay_equals_eager_calls(N, W, M):
    """`capture_fused_crowd_ws`: the K-step launch as a one-node hipGraph; replays advance the device-side counters like eager calls -- one
    more step() on each side lands in the same ring block and draws the same actions only if both counters agree."""
    env_a, _, _, a = _make(W, N, M, 3, **FAST)
    env_b, _, _, b = _make(W, N, M, 3, **FAST)
    a.capture_fused_crowd_ws(steps_per_graph=4)       # (runs 2 warm-up steps outside the capture)
    b.run_fused_crowd_ws(2)
    a.replay(3)
    for _ in range(3):
        b.run_fused_crowd_ws(4)
    _compare(env_a, a, env_b, b, 14)
    a.step(); b.step()                                # the rollout's and the policy's device-side step counters: what the next step starts from
    _compare(env_a, a, env_b, b, 15)
    assert (a.emit_t >= 0).any()
    with pytest.raises(ValueError):
        a.capture_fused_crowd_ws(steps_per_graph=3)
    _close((env_a, a), (env_b, b))


def _run(env, roll, pol, n_steps=2, same_buffer=False):
    from rl_collision_avoidance_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr())
    b = roll._actor_buffers()
    cur, nxt = roll._obs_buffers[roll._cur], roll._obs_buffers[roll._cur if same_buffer else 1 - roll._cur]
    rc = _lib.lib().cavoid_crowd_actor_run_ws(env._h, pol._h, roll._h, C.byref(b), p(cur), p(nxt), p(env.rewards), p(env.done), p(env.game_over),
                                              p(roll._act_out), p(roll._val_out), n_steps, 0, None)
    torch.cuda.synchronize()
    return rc


def test_fused_crowd_ws_actor_refuses_what_it_does_not_carry():
    made = []

    def refused(code, word, *args, **kw):
        env, _, pol, roll = _make(*args, **kw)
        made.append((env, roll))
        why = roll.crowd_ws_fused_unavailable_reason
        assert why is not None and word in why, why
        assert not roll.crowd_ws_fused_available
        with pytest.raises(RuntimeError) as err:
            roll.run_fused_crowd_ws(2)
        assert why in str(err.value)
        assert _run(env, roll, pol) == code                  # straight at the C ABI: a code, not a crash
        return roll
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
    before = [t.clone() for t in tensors()]
    assert _run(env, roll, pol, n_steps=0) == OK
    assert all(torch.equal(u, v) for u, v in zip(before, tensors()))
    # ... and a same-buffer call is an argument error, as for cavoid_actor_run
    assert _run(env, roll, pol, same_buffer=True) == EINVAL
    assert all(torch.equal(u, v) for u, v in zip(before, tensors()))
    _close(*made)


def _train(tmp_path, extra):
    cmd = [sys.executable, "-m", "rl_collision_avoidance_amd.ga3c.train", "--agents", "20", "--arch", "weight_sharing", "--worlds", "64",
           "--episodes", "300", "--pretrain-steps", "0", "--print-every", "100", "--train-rows", "2048",
           "--checkpoint-dir", str(tmp_path / "ck")] + extra
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    run = subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-3000:])
    return run


def test_train_cli_with_the_flag_runs_the_crowd_ws_actor_kernel(tmp_path):
    run = _train(tmp_path, ["--fused-crowd-ws-actor"])
    assert run.returncode == 0
    assert "actors: fused crowd weight_sharing actor kernel (cavoid_crowd_actor_run_ws), 4 env steps per launch" in run.stdout
    assert "finished" in run.stdout and " 0 training steps" not in run.stdout


def test_train_cli_without_the_flag_prints_todays_line(tmp_path):
    run = _train(tmp_path, [])
    assert run.returncode == 0
    assert ("actors: one launch per phase (policy, env + bookkeeping) -- fused kernel not applicable: more than 16 agents per world "
            "(the crowd step form has no fused actor kernel); in a hipGraph, 4 env steps per graph") in run.stdout
    assert "cavoid_crowd_actor_run_ws" not in run.stdout and "finished" in run.stdout


def test_train_cli_with_the_flag_ends_where_the_kernel_does_not_apply(tmp_path):
    """with a reason the run ends with SystemExit naming it (in this process: nothing is captured or trained before that)"""
    from rl_collision_avoidance_amd.ga3c import train
    with pytest.raises(SystemExit, match="--fused-crowd-ws-actor.*not a FusedPolicy"):
        train.main(["--agents", "20", "--arch", "weight_sharing", "--worlds", "64", "--episodes", "64", "--pretrain-steps", "0", "--print-every", "0",
                    "--train-rows", "2048", "--checkpoint-dir", str(tmp_path / "ck"), "--fused-crowd-ws-actor", "--torch-policy"])
