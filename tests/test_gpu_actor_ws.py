"""GPU tests of the weight_sharing network's fused actor kernel (`cavoid_actor_run_ws`, csrc/cavoid_actor_ws.hpp): K closed-loop GA3C actor
steps -- the weight_sharing pass, action selection, env.step, Experience bookkeeping -- in ONE launch, against the same K steps taken one
launch at a time (BatchedRollout.step: `cavoid_rollout_active_rows`, `cavoid_policy_forward[_rows]` on the weight_sharing handle,
`cavoid_step_push`).  The fused kernel runs the very same statements per value, so everything must be BIT-identical: observations, world
state, episode counters, the experience rings (state rows, values, returns, actions, emission stamps), the training rows handed to the
trainer; only the episode totals are compared to float32 rounding (they are accumulated with unordered atomics in both forms).

The step-by-step form itself is pinned elsewhere: the weight_sharing kernels against PyTorch (test_gpu_policy_ws.py), env and rollout
against the oracle and the reference's goldens (test_gpu_parity.py, test_gpu_rollout.py)."""
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
KS = (2, 1, 7, 16, 4) + (16,) * 14 + (3,)                    # odd counts too: the observation buffers alternate
OK, EINVAL, EUNSUPPORTED = 0, -1, -4


def _make(W, N, M, seed, reflush=False, greedy=False, arch="weight_sharing", net_M=None, ws_crowd=False, time_max=5, **over):
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.config import EnvConfig
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout

    class Cfg(EnvConfig):
        def __init__(self, m):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = m
            EnvConfig.__init__(self)
    cfg = Cfg(M)
    env = BatchedCollisionAvoidanceEnv(W, cfg, device="cuda:0", seed=seed, **over)
    torch.manual_seed(1234)
    net = NetworkVP_rnn(cfg if net_M is None else Cfg(net_M), arch=arch).to("cuda:0")
    pol = FusedPolicy(net, seed=77, ws_crowd=ws_crowd)
    # skip_finished = not reflush: the fused kernel hands a result only to the rows that still need an action (with the re-flush quirk: to
    # every row), exactly the rows the step-by-step path lists with skip_finished -- like is compared with like.  Short chunks: many
    # flushes; room for every duplicate row of the re-flush quirk (a full buffer drops rows in arrival order, which legitimately differs).
    roll = BatchedRollout(env, pol, reflush_done=reflush, greedy=greedy, time_max=time_max, dup_capacity=600000 if reflush else None,
                          skip_finished=not reflush)
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
    for name in ("x", "val", "ret", "act_ring", "emit_t"):
        _same(getattr(a, name), getattr(b, name), (name, total))
    assert a.step_index == b.step_index == total


def _close(*pairs):
    for env, roll in pairs:
        roll.close(); env.close()


# (N, W, M, settings): the smallest shapes at which each part can go wrong
@pytest.mark.parametrize("N,W,M,over", [
    # the WS-8 shape: M > N - 1 (slots past the count carry is_on = 0), ragged last tile (8 tiles + 2 worlds), quad env step
    (4, 130, 7, dict()),
    # 63-row tiles, every row counts, scripted agents, ragged tile
    (3, 45, 2, dict(reflush=True, gen_min_agents=2, gen_nonlearning_fraction=0.3)),
    # 60-row tiles, the widest parked row (M = kWsMaxOthers), single-wavefront env step
    (10, 20, 19, dict(gen_min_agents=2, gen_nonlearning_fraction=0.2)),
    # clip to M < N - 1, argmax, generator inside the step
    (6, 40, 3, dict(greedy=True, gen_pool_size=0, gen_min_agents=5)),
    # actor_ws_kernel<N, true>: ORCA agents
    (4, 100, 7, dict(rvo_enabled=1, gen_rvo_fraction=0.5, gen_nonlearning_fraction=0.5, gen_min_agents=2)),
    # box scenarios generated in the step (the RVO form without ORCA agents)
    (3, 60, 4, dict(reflush=True, gen_mode=1, gen_pool_size=0)),
    # N = 2, M = 1, pool scenarios
    (2, 64, 1, dict(gen_mode=1, gen_pool_size=200)),
    # closest_first, the WS baselines' own order
    (4, 500, 7, dict(sort_method=1, gen_min_agents=3)),
    # 512 tiles: two workgroups per CU, one tile's env step under another's matrix phase
    (4, 8192, 7, dict()),
    # WS-8 at 4 agents with the backward pass past its 32 registers (the serial form), and with all 32 live
    (4, 130, 7, dict(time_max=33)),
    (4, 130, 7, dict(time_max=33, reflush=True, gen_min_agents=2, gen_nonlearning_fraction=0.3)),
    (4, 130, 7, dict(time_max=31)),
])
def test_fused_ws_actor_equals_step_by_step(N, W, M, over):
    over = dict(over)
    reflush, greedy = over.pop("reflush", False), over.pop("greedy", False)
    seed = 21
    env_a, net_a, _, a = _make(W, N, M, seed, reflush, greedy, **over)
    env_b, net_b, _, b = _make(W, N, M, seed, reflush, greedy, **over)
    assert a.ws_fused_available, a.ws_fused_unavailable_reason
    assert not a.fused_available                             # (the default paths do not change)
    for p, q in zip(net_a.parameters(), net_b.parameters()):
        assert torch.equal(p, q)
    _same(a.obs, b.obs, "first observation")
    total = 0
    for k in KS:
        a.run_fused_ws(k)
        for _ in range(k):
            b.step()
        total += k
        if total > 40 and total % 64:                        # (full comparisons early on, then every fourth launch)
            continue
        _compare(env_a, a, env_b, b, total)
    _compare(env_a, a, env_b, b, total)
    assert env_a.episode.max().item() >= 1                   # restarts are inside what was compared
    # what reaches the trainer and the stats process
    ba, bb = a.drain(flush_all=True), b.drain(flush_all=True)
    assert len(ba) == len(bb) > 0 and ba.dropped == bb.dropped == 0
    if over.get("time_max", 5) > 5:
        rs.require_deep_flushes(bb.src.cpu().numpy(), over["time_max"], "ws actor N=%d W=%d reflush=%s" % (N, W, reflush))
    ka = np.lexsort(ba.src.cpu().numpy().T[::-1])
    kb = np.lexsort(bb.src.cpu().numpy().T[::-1])
    for name in ("src", "x", "r", "a_index"):
        assert np.array_equal(getattr(ba, name).cpu().numpy()[ka], getattr(bb, name).cpu().numpy()[kb]), name
    ea, eb = a.drain_episodes().cpu().numpy(), b.drain_episodes().cpu().numpy()
    assert len(ea) == len(eb) > 0
    ea, eb = ea[np.lexsort(ea.T[::-1])], eb[np.lexsort(eb.T[::-1])]
    assert np.array_equal(ea[:, 0], eb[:, 0]) and np.array_equal(ea[:, 2], eb[:, 2])
    np.testing.assert_allclose(ea[:, 1], eb[:, 1], rtol=1e-6, atol=1e-6)
    # and the two forms interleave: each continues where the other stopped
    a.step(); a.run_fused_ws(3)
    b.run_fused_ws(2); b.step(); b.step()
    _same(a.obs, b.obs, "interleaved obs")
    _same(a.emit_t, b.emit_t, "interleaved emit_t")
    _close((env_a, a), (env_b, b))


def _run(env, roll, pol, n_steps=2):
    from rl_collision_avoidance_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr())
    b = roll._actor_buffers()
    cur, nxt = roll._obs_buffers[roll._cur], roll._obs_buffers[1 - roll._cur]
    rc = _lib.lib().cavoid_actor_run_ws(env._h, pol._h, roll._h, C.byref(b), p(cur), p(nxt), p(env.rewards), p(env.done), p(env.game_over),
                                        p(roll._act_out), p(roll._val_out), n_steps, 0, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("N", range(1, 17))
def test_availability_agrees_with_the_entry_point_for_every_agent_count(N):
    """Which agent counts the 66 560 lent bytes carry: `ws_fused_available` says what `cavoid_actor_run_ws` returns, and where it runs, it
    equals the step-by-step path."""
    W, M = 2 * (64 // N) + 1, min(N - 1, 7) or 1
    env_a, _, pol_a, a = _make(W, N, M, 3)
    env_b, _, _, b = _make(W, N, M, 3)
    rc = _run(env_a, a, pol_a, n_steps=5)
    assert rc in (OK, EUNSUPPORTED) and (rc == OK) == a.ws_fused_available, (rc, a.ws_fused_unavailable_reason)
    if rc == OK:
        a._cur, a.step_index = (a._cur + 5) & 1, a.step_index + 5      # (what run_fused_ws(5) keeps on the host)
        for _ in range(5):
            b.step()
        _compare(env_a, a, env_b, b, 5)
    _close((env_a, a), (env_b, b))


def test_fused_ws_actor_graph_replay_equals_eager_calls():
    """`capture_fused_ws`: the K-step launch as a one-node hipGraph; replays advance the device-side counters like eager calls."""
    env_a, _, _, a = _make(130, 4, 7, 3)
    env_b, _, _, b = _make(130, 4, 7, 3)
    a.capture_fused_ws(steps_per_graph=4)        # (runs 2 warm-up steps outside the capture)
    b.run_fused_ws(2)
    a.replay(6)
    for _ in range(6):
        b.run_fused_ws(4)
    _compare(env_a, a, env_b, b, 26)
    _close((env_a, a), (env_b, b))


def test_a_masked_reset_between_two_fused_ws_launches_needs_no_flag_fixup():
    """done / game_over are OUTPUTS of cavoid_actor_run_ws: which rows need an action at a launch's first step is derived from the world
    state.  A masked reset between two launches leaves them stale for the reset worlds; launch 2 must give those agents real actions all the
    same -- identical to a twin whose buffers were patched to what a step that restarted those worlds would have left."""
    W, N, M, seed, K1 = 2048, 4, 7, 9, 40                    # (K1 even: the current observation is back in env.obs)
    env_a, _, _, a = _make(W, N, M, seed)
    env_b, _, _, b = _make(W, N, M, seed)
    for r in (a, b):
        r.run_fused_ws(K1)
    _same(a.obs, b.obs, "after launch 1")
    stale = (env_a.done.bool() & (a.obs[..., 0] > 0.5)).any(dim=1) & (env_a.game_over == 0)
    assert int(stale.sum()) >= 5
    mask = stale.to(torch.uint8)
    for env in (env_a, env_b):
        env.reset(mask)
    env_b.done[stale] = 0
    env_b.game_over[stale] = 1
    assert not torch.equal(env_a.done, env_b.done)
    for r in (a, b):
        r.run_fused_ws(6)
    _same(a.obs, b.obs, "obs after launch 2")
    for x, y in zip(env_a.get_state(), env_b.get_state()):
        _same(x, y, "state after launch 2")
    for name in ("x", "val", "ret", "act_ring", "emit_t"):
        _same(getattr(a, name), getattr(b, name), name)
    t0 = K1 % a.ring_len
    acted = a.act_ring[t0].view(W, N)[stale]
    assert int((acted != 0).sum()) > 0
    _close((env_a, a), (env_b, b))


def test_rows_that_need_no_action_get_none():
    """Right after a reset every learning agent needs an action -- scripted and absent agents' rows are handed action 0 / value 0 -- and a
    live row's value is bit for bit the stand-alone pass's on the same observation, whatever tile row the row list moved it to."""
    W, N = 300, 4
    env, net, pol, roll = _make(W, N, 7, 5, gen_min_agents=2, gen_nonlearning_fraction=0.5, gen_static_fraction=0.5)
    obs0 = roll.obs.clone()
    need = (obs0[..., 0] > 0.5)
    assert 0.2 < need.float().mean().item() < 0.8
    roll.run_fused_ws(1)
    torch.cuda.synchronize()
    acts, vals = roll._act_out.view(W, N), roll._val_out.view(W, N)
    assert (acts[~need] == 0).all() and (vals[~need] == 0).all()
    _, v_ref = pol(obs0[..., 1:].reshape(W * N, -1))         # the stand-alone kernel on every row
    assert torch.equal(vals[need], v_ref.view(W, N)[need])
    assert (acts[need] >= 0).all() and (acts[need] < env.num_actions).all() and acts[need].float().std().item() > 0
    _close((env, roll))


def test_fused_ws_actor_refuses_what_it_does_not_carry():
    made = []

    def refused(word, *args, **kw):
        env, _, pol, roll = _make(*args, **kw)
        made.append((env, roll))
        why = roll.ws_fused_unavailable_reason
        assert why is not None and word in why, why
        with pytest.raises(RuntimeError) as err:
            roll.run_fused_ws(2)
        assert why in str(err.value)
        assert _run(env, roll, pol) == EUNSUPPORTED          # straight at the C ABI: a code, not a crash
    refused("rnn network", 32, 4, 3, 1, arch="rnn")
    refused("ring", 32, 4, 24, 1, ws_crowd=True)             # a 4-agent env padded to M = 24: the ring handle
    refused("20 agents per world", 8, 20, 7, 1)
    refused("holonomic", 32, 4, 7, 1, dynamics=2)
    # an env whose generator makes frozen-network agents (the rollout insists on a frozen_policy for it: the learner's handle serves)
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    env, _, pol, roll = _make(32, 4, 7, 1)
    made.append((env, roll))
    env_f = BatchedCollisionAvoidanceEnv(32, env.config, device="cuda:0", seed=1, gen_min_agents=2, gen_nonlearning_fraction=0.5, gen_frozen_fraction=0.5)
    roll_f = BatchedRollout(env_f, pol, time_max=5, skip_finished=True, frozen_policy=pol)
    roll_f.reset()
    made.append((env_f, roll_f))
    assert "frozen-network agents" in roll_f.ws_fused_unavailable_reason
    with pytest.raises(RuntimeError, match="frozen-network agents"):
        roll_f.run_fused_ws(2)
    assert _run(env_f, roll_f, pol) == EUNSUPPORTED
    # a handle whose M differs from the env's: an argument error; n_steps = 0: CAVOID_OK, and nothing changes
    env_m, _, pol_m, roll_m = _make(32, 4, 7, 1, net_M=3)
    made.append((env_m, roll_m))
    assert "the env's rows carry 7" in roll_m.ws_fused_unavailable_reason and _run(env_m, roll_m, pol_m) == EINVAL
    roll.run_fused_ws(3)
    before = [t.clone() for t in (roll._obs_buffers[0], roll._obs_buffers[1], roll.x, roll.emit_t, env.episode, env.rewards, *env.get_state())]
    assert _run(env, roll, pol, n_steps=0) == OK
    after = [roll._obs_buffers[0], roll._obs_buffers[1], roll.x, roll.emit_t, env.episode, env.rewards, *env.get_state()]
    assert all(torch.equal(u, v) for u, v in zip(before, after))
    _close(*made)


def _train(tmp_path, extra):
    cmd = [sys.executable, "-m", "rl_collision_avoidance_amd.ga3c.train", "--arch", "weight_sharing", "--agents", "4", "--worlds", "64",
           "--episodes", "300", "--pretrain-steps", "0", "--print-every", "100", "--train-rows", "2048",
           "--checkpoint-dir", str(tmp_path / "ck")] + extra
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    run = subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-3000:])
    return run


def test_train_cli_with_the_flag_runs_the_ws_actor_kernel(tmp_path):
    run = _train(tmp_path, ["--fused-ws-actor"])
    assert run.returncode == 0
    assert "actors: fused weight_sharing actor kernel (cavoid_actor_run_ws), 4 env steps per launch" in run.stdout
    assert "finished" in run.stdout and " 0 training steps" not in run.stdout


def test_train_cli_without_the_flag_prints_todays_line(tmp_path):
    run = _train(tmp_path, [])
    assert run.returncode == 0
    assert ("actors: one launch per phase (policy, env + bookkeeping) -- fused kernel not applicable: the policy is the weight_sharing network "
            "(the fused actor kernel embeds the LSTM pass; its kernel acts step by step); in a hipGraph, 4 env steps per graph") in run.stdout
    assert "cavoid_actor_run_ws" not in run.stdout and "finished" in run.stdout


def test_train_cli_with_the_flag_ends_where_the_kernel_does_not_apply(tmp_path):
    run = _train(tmp_path, ["--fused-ws-actor", "--scripted-fraction", "0.5", "--frozen-fraction", "0.5"])
    assert run.returncode != 0
    assert "--fused-ws-actor: the weight_sharing actor kernel (cavoid_actor_run_ws) does not apply: frozen-network agents" in run.stdout
    assert "actors:" not in run.stdout
