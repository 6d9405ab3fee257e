"""GPU tests of the weight_sharing network's fused actor kernel (`cavoid_actor_run_ws`, csrc/cavoid_actor_ws.hpp): K closed-loop GA3C actor
steps -- the weight_sharing pass, action selection, env.step, Experience bookkeeping -- in ONE launch, against the same K steps taken one
launch at a time (BatchedRollout.step: `cavoid_rollout_active_rows`, `cavoid_policy_forward[_rows]` on the weight_sharing handle,
`cavoid_step_push`).  The fused kernel runs the very same statements per value, so everything must be BIT-identical: observations, world
state, episode counters, the experience rings (state rows, values, returns, actions, emission stamps), the training rows handed to the
trainer; only the episode totals are compared to float32 rounding (they are accumulated with unordered atomics in both forms).

The step-by-step form itself is pinned elsewhere: the weight_sharing kernels against PyTorch (test_gpu_policy_ws.py), env and rollout
against the oracle and the reference's goldens (test_gpu_parity.py, test_gpu_rollout.py)."""
import pytest

torch = pytest.importorskip("torch")

from tests import actor_twins as tw
from tests.actor_twins import KS_TILE as KS, close as _close, same as _same
from tests.gpu_support import EINVAL, EUNSUPPORTED, OK

pytestmark = pytest.mark.gpu

ARGS = ["--arch", "weight_sharing", "--agents", "4"]        # the train CLI's shape in this file


def _make(W, N, M, seed, reflush=False, greedy=False, arch="weight_sharing", net_M=None, ws_crowd=False, time_max=5, **over):
    # short chunks: many flushes; the handle is the whole-row one unless a case asks for the ring handle
    return tw.make(W, N, M, seed, reflush, greedy, arch=arch, net_M=net_M, ws_crowd=ws_crowd, time_max=time_max, **over)


def _compare(env_a, a, env_b, b, total):
    tw.compare_twins(env_a, a, env_b, b, total, rings=tw.RINGS)         # (this form's tests never compared dup_count)


def _run(env, roll, pol, n_steps=2):
    return tw.raw_run(tw.TILE_WS, env, roll, pol, n_steps)


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
    twin_a, twin_b = _make(W, N, M, 21, reflush, greedy, **over), _make(W, N, M, 21, reflush, greedy, **over)
    a = twin_a[3]
    assert a.ws_fused_available, a.ws_fused_unavailable_reason
    assert not a.fused_available                             # (the default paths do not change)
    time_max = over.get("time_max", 5)
    tw.fused_equals_step_by_step(
        tw.TILE_WS, twin_a, twin_b, ("ws actor", N, W, M, reflush), ks=KS,
        compare_at=lambda total: total <= 40 or total % 64 == 0,         # (full comparisons early on, then every fourth launch)
        compare_at_end=True, rings=tw.RINGS,                             # (restarts are inside what was compared; no dup_count in this form's test)
        deep_flushes=(time_max, "ws actor N=%d W=%d reflush=%s" % (N, W, reflush)) if time_max > 5 else None,
        interleave=tw.INTERLEAVE_TILE)


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
    twin_a, twin_b = _make(130, 4, 7, 3), _make(130, 4, 7, 3)
    tw.graph_replay(tw.TILE_WS, twin_a, twin_b, 6, _compare)            # (compared at step 2 + 6 * 4 = 26)
    _close((twin_a[0], twin_a[3]), (twin_b[0], twin_b[3]))


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
        tw.refused(tw.TILE_WS, env, pol, roll, EUNSUPPORTED, word, reason_in_error=True)
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
    tensors = lambda: (roll._obs_buffers[0], roll._obs_buffers[1], roll.x, roll.emit_t, env.episode, env.rewards, *env.get_state())
    assert tw.unchanged_by(lambda: _run(env, roll, pol, n_steps=0), tensors, "cavoid_actor_run_ws with n_steps = 0") == OK
    _close(*made)


def test_train_cli_with_the_flag_runs_the_ws_actor_kernel(tmp_path):
    tw.train_cli_runs_the_kernel(tmp_path, ARGS + ["--fused-ws-actor"],
                                 "actors: fused weight_sharing actor kernel (cavoid_actor_run_ws), 4 env steps per launch")


def test_train_cli_without_the_flag_prints_todays_line(tmp_path):
    tw.train_cli_prints_todays_line(
        tmp_path, ARGS,
        "actors: one launch per phase (policy, env + bookkeeping) -- fused kernel not applicable: the policy is the weight_sharing network "
        "(the fused actor kernel embeds the LSTM pass; its kernel acts step by step); in a hipGraph, 4 env steps per graph", "cavoid_actor_run_ws")


def test_train_cli_with_the_flag_ends_where_the_kernel_does_not_apply(tmp_path):
    run = tw.train_cli(tmp_path, ARGS + ["--fused-ws-actor", "--scripted-fraction", "0.5", "--frozen-fraction", "0.5"])
    assert run.returncode != 0
    assert "--fused-ws-actor: the weight_sharing actor kernel (cavoid_actor_run_ws) does not apply: frozen-network agents" in run.stdout
    assert "actors:" not in run.stdout
