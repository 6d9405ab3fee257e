"""GPU tests of the fused actor kernel (`cavoid_actor_run`, csrc/cavoid_actor.hpp): K closed-loop GA3C actor steps -- policy
forward, action selection, env.step, Experience bookkeeping -- in ONE launch, against the same K steps taken one launch at a
time through `cavoid_policy_forward` + `cavoid_step_autoreset` + `cavoid_rollout_push` (BatchedRollout.step).  The fused kernel
runs the very same statements per value, so everything must be BIT-identical: observations, world state, episode counters,
the experience rings (state rows, rewards, returns, actions, emission stamps), the training rows handed to the trainer; only
the episode totals are compared to float32 rounding (the step-by-step form accumulates them with unordered atomics).

The step-by-step form itself is pinned elsewhere: env vs the float64 oracle (test_gpu_parity.py), rollout vs the reference's
own ProcessAgent goldens (test_gpu_rollout.py), policy vs PyTorch fp32 (test_gpu_policy.py)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import actor_twins as tw
from tests import rollout_scripts as rs
from tests.actor_twins import same as _same
from tests.gpu_support import EINVAL, EUNSUPPORTED

pytestmark = pytest.mark.gpu


def _make(W, N, seed, reflush, greedy=False, skip_finished=None, M=None, time_max=5, **over):
    # The fused kernel runs the network only for the rows that still need an action (a learning agent that has not finished; with the
    # re-flush quirk or frozen-network agents: every row), exactly the rows the step-by-step path lists with skip_finished -- what a
    # finished agent's ring entry holds as action is whatever it was last given, in both forms, so the forms are compared like for like.
    if skip_finished is None:
        skip_finished = (not reflush) and not (over.get("gen_frozen_fraction", 0.0) > 0.0)
    # short chunks: many flushes; the frozen-network agents' network where the generator makes them
    return tw.make(W, N, M, seed, reflush, greedy, frozen="from_fraction", skip_finished=skip_finished, time_max=time_max, **over)


@pytest.mark.parametrize("N,W,reflush,greedy,over", [
    (4, 512, False, False, dict()),                                     # BASELINE configs[4] shape (32 tiles)
    (4, 1000, True, False, dict(gen_min_agents=2, gen_nonlearning_fraction=0.3)),    # the reference's re-flush quirk, scripted agents, ragged last tile
    (10, 300, False, False, dict(gen_min_agents=2, gen_nonlearning_fraction=0.2)),   # configs[3] shape (6 worlds per tile, 4 idle rows)
    (3, 130, False, True, dict(gen_pool_size=0)),                       # greedy (PLAY_MODE), in-kernel scenario generator
    (2, 64, False, False, dict(gen_mode=1, gen_pool_size=200)),         # box scenarios from the pool
    (4, 700, False, False, dict(rvo_enabled=1, gen_rvo_fraction=0.5, gen_nonlearning_fraction=0.5, gen_min_agents=2)),   # ORCA agents (actor_kernel<N, true>)
    (3, 200, True, False, dict(gen_mode=1, gen_pool_size=0)),           # box scenarios generated inside the step
    (10, 100, False, False, dict(rvo_enabled=1, gen_mode=1, gen_pool_size=0, gen_rvo_fraction=0.5, gen_nonlearning_fraction=0.4, gen_min_agents=3)),
    # frozen-network agents (scripted policy 4: the GA3C-CADRL agent mechanism) inside the fused launch -- cavoid_actor_run_mix
    (4, 600, False, False, dict(gen_min_agents=2, gen_nonlearning_fraction=0.6, gen_static_fraction=0.2, gen_frozen_fraction=0.6)),
    # ... the reference's whole training mix: static / non-cooperative / RVO / frozen network, box scenarios generated in the step
    (4, 500, True, False, dict(rvo_enabled=1, gen_mode=1, gen_pool_size=0, gen_min_agents=2, gen_nonlearning_fraction=0.7, gen_static_fraction=0.2,
                               gen_rvo_fraction=0.3, gen_frozen_fraction=0.3)),
    (10, 200, False, True, dict(gen_min_agents=3, gen_nonlearning_fraction=0.5, gen_static_fraction=0.1, gen_frozen_fraction=0.8, gen_pool_size=300)),
    # full-size batches: TWO workgroups per compute unit, so a tile's env step shares its SIMD with the other tile's matrix phase --
    # the only place a packed-float32 operand-swap pattern in the env step ever misbehaved (round 4; tools/repro_actor_case.py)
    (4, 8192, False, False, dict(rvo_enabled=1, gen_rvo_fraction=1.0, gen_nonlearning_fraction=0.7, gen_pool_size=20000)),
    (4, 8192, False, False, dict()),
    (10, 4096, False, False, dict(gen_min_agents=2)),
    # the env step's configuration space inside the fused kernel: the clip to M < N - 1 neighbours, the other sort orders, the
    # U7 / U2 switches, the max-turn-rate dynamics
    (4, 600, False, False, dict(M=2, gen_min_agents=4)),
    (6, 300, False, False, dict(M=3, gen_min_agents=5, gen_nonlearning_fraction=0.2)),
    (4, 500, False, False, dict(sort_method=1, gen_min_agents=3)),                  # closest_first
    (5, 400, False, False, dict(sort_method=2, gen_min_agents=2)),                  # time_to_impact
    (4, 500, False, False, dict(sort_round_gap=0, sort_tie_lateral=0, wrap_closed_end=1)),
    # unicycle_max_turn_rate, with turns the clamp cuts (the default table's widest, pi/6, is below max_turn_rate * dt)
    (4, 500, False, False, dict(dynamics=1, gen_min_agents=2, actions=[[1.0, 0.3], [1.0, -0.3], [1.0, 0.0], [1.0, 0.9], [1.0, -0.9], [0.5, 1.2],
                                                                      [0.5, -1.2], [0.0, 0.7], [0.0, -0.7], [1.0, 1.5], [1.0, -1.5]])),
    # the backward pass past its 32 registers (time_max + 1 > 32: the serial form) and with all 32 live (time_max = 31), 8 tiles
    (4, 128, False, False, dict(time_max=33)),
    (4, 128, True, False, dict(time_max=33, gen_min_agents=2, gen_nonlearning_fraction=0.3)),
    (4, 128, False, False, dict(time_max=31)),
])
def test_fused_actor_equals_step_by_step(N, W, reflush, greedy, over):
    twin_a, twin_b = _make(W, N, 21, reflush, greedy, **over), _make(W, N, 21, reflush, greedy, **over)
    a = twin_a[3]
    assert a.fused_available and a.actor_path.startswith("fused actor kernel"), a.actor_path
    time_max = over.get("time_max", 5)
    tw.fused_equals_step_by_step(
        tw.TILE, twin_a, twin_b, ("fused actor", N, W, reflush), ks=tw.KS_TILE,
        compare_at=lambda total: total <= 40 or total % 64 == 0,         # (full comparisons early on, then every fourth launch)
        rings=tw.RINGS,                                                  # (this form's test never compared dup_count)
        deep_flushes=(time_max, "fused actor N=%d W=%d reflush=%s" % (N, W, reflush)) if time_max > 5 else None,
        interleave=tw.INTERLEAVE_TILE)                                   # (... and its interleave looks at obs and emit_t)


def test_fused_actor_equals_step_by_step_with_a_row_list():
    """`skip_finished` (the step-by-step path runs the policy on the rows that still need an action only; batches above 65 536 rows
    choose it by themselves) changes nothing the fused kernel could differ in: it stays available and equal."""
    W, N, seed = 700, 4, 5
    env_a, _, _, a = _make(W, N, seed, False, skip_finished=True, gen_min_agents=2, gen_nonlearning_fraction=0.3)
    env_b, _, _, b = _make(W, N, seed, False, skip_finished=True, gen_min_agents=2, gen_nonlearning_fraction=0.3)
    assert a.fused_available and b.skip_finished
    for k in (3, 16, 16, 16, 16, 16, 16, 16, 16, 16, 5):
        a.run_fused(k)
        for _ in range(k):
            b.step()
        _same(a.obs, b.obs, "obs")
        for x, y in zip(env_a.get_state(), env_b.get_state()):
            _same(x, y, "state")
        # (the action / value rings hold whatever the policy put out for EVERY slot; for agents that are finished and wait, the row
        #  list leaves the previous entry -- never read -- so the rings are compared through what becomes a training row)
        for name in ("x", "emit_t"):
            _same(getattr(a, name), getattr(b, name), name)
    ba, bb = a.drain(flush_all=True), b.drain(flush_all=True)
    assert len(ba) == len(bb) > 0
    tw.compare_drained(ba, bb, "fused actor with a row list")
    tw.close((env_a, a), (env_b, b))


def test_fused_actor_graph_replay_equals_eager_calls():
    """`capture_fused`: the K-step launch as a one-node hipGraph; replays advance the device-side counters like eager calls."""
    W, N, seed = 256, 4, 3
    twin_a, twin_b = _make(W, N, seed, False), _make(W, N, seed, False)

    def compare(env_a, a, env_b, b, total):
        _same(a.obs, b.obs, "obs")
        for name in ("x", "ret", "emit_t"):
            _same(getattr(a, name), getattr(b, name), name)
        assert a.step_index == b.step_index == total == 14
    tw.graph_replay(tw.TILE, twin_a, twin_b, 3, compare)
    tw.close((twin_a[0], twin_a[3]), (twin_b[0], twin_b[3]))


def test_fused_actor_refuses_what_it_does_not_carry():
    env, _, pol, roll = _make(64, 4, 1, False, dynamics=2)             # velocity (holonomic) actions: the step-by-step entry points carry them
    assert not roll.fused_available and "holonomic" in roll.actor_path
    with pytest.raises(RuntimeError):
        roll.run_fused(2)
    # straight at the C ABI: a code, not a crash
    assert tw.raw_run(tw.TILE, env, roll, pol, cur=0) == EUNSUPPORTED
    assert tw.raw_run(tw.TILE, env, roll, pol, cur=0, same_buffer=True) == EINVAL
    roll.close(); env.close()
    # an env whose generator makes frozen-network agents: cavoid_actor_run (no second network) refuses it, cavoid_actor_run_mix carries it
    env, _, pol, roll = _make(64, 4, 1, False, gen_min_agents=2, gen_nonlearning_fraction=0.5, gen_frozen_fraction=0.5)
    assert roll.fused_available and "cavoid_actor_run_mix" in roll.actor_path
    assert tw.raw_run(tw.TILE, env, roll, pol, cur=0) == EUNSUPPORTED
    roll.run_fused(2)
    roll.close(); env.close()


def test_pipelined_hand_over_equals_drain():
    """`drain_begin` / `drain_end` (the count of hand-over k is read while launch k+1 runs) deliver the rows `drain()` delivers."""
    W, N, seed = 512, 4, 9
    env_a, _, _, a = _make(W, N, seed, False)
    env_b, _, _, b = _make(W, N, seed, False)
    rows_a, rows_b, pending = [], [], None
    for _ in range(12):
        a.run_fused(8)
        rows_a.append(a.drain(provenance=True))
        b.run_fused(8)
        h = b.drain_begin(provenance=True)
        if pending is not None:
            rows_b.append(b.drain_end(pending))
        pending = h
    rows_b.append(b.drain_end(pending))
    assert a.frames == b.frames > 0
    for name in ("x", "r", "a_index", "src"):
        xa = torch.cat([getattr(r, name) for r in rows_a]).cpu().numpy()
        xb = torch.cat([getattr(r, name) for r in rows_b]).cpu().numpy()
        sa = torch.cat([r.src for r in rows_a]).cpu().numpy()
        sb = torch.cat([r.src for r in rows_b]).cpu().numpy()
        assert np.array_equal(xa[np.lexsort(sa.T[::-1])], xb[np.lexsort(sb.T[::-1])]), name
    with pytest.raises(RuntimeError):
        _make(64, 4, 1, True)[3].drain_begin()
    for r in (a, b):
        r.close()
    env_a.close(); env_b.close()


@pytest.mark.parametrize("N,W,reflush,over", [
    (4, 1000, True, dict(gen_min_agents=2, gen_nonlearning_fraction=0.3)),
    (10, 300, False, dict(gen_min_agents=2, gen_nonlearning_fraction=0.2)),
    (4, 500, False, dict(rvo_enabled=1, gen_rvo_fraction=0.5, gen_nonlearning_fraction=0.5, gen_mode=1, gen_pool_size=0)),
    (1, 200, False, dict()),
    (4, 300, True, dict(time_max=33, gen_min_agents=2, gen_nonlearning_fraction=0.3)),      # the serial backward pass
    (4, 300, False, dict(time_max=33)),
    (4, 300, False, dict(time_max=31)),                                                      # all 32 registers live
])
def test_step_push_equals_step_then_push(N, W, reflush, over):
    """`cavoid_step_push` (env.step + Experience bookkeeping in ONE launch, BatchedRollout.step's default) against the three launches
    it replaces (`cavoid_step_autoreset`, `cavoid_rollout_push`: push + episode log), bitwise; scripted actions / values (N = 1 has
    no policy to run) and, for N > 1, the policy in the loop."""
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.config import EnvConfig
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            EnvConfig.__init__(self)
    over = dict(over)
    time_max = over.pop("time_max", 5)
    rolls = []
    for fuse in (True, False):
        if N > 1:
            env, _, _, roll = _make(W, N, 17, reflush, False, time_max=time_max, **over)
        else:
            env = BatchedCollisionAvoidanceEnv(W, Cfg(), device="cuda:0", seed=17, **over)
            roll = BatchedRollout(env, None, reflush_done=reflush, time_max=time_max)
            roll.reset()
        roll.fuse_env_push = fuse
        rolls.append((env, roll))
    (ea, a), (eb, b) = rolls
    g = torch.Generator(device="cuda").manual_seed(3)
    for t in range(150):
        if N > 1 and t % 3:
            a.step(); b.step()                               # policy in the loop
        else:
            acts = torch.randint(0, 11, (W, N), generator=g, device="cuda", dtype=torch.int32)
            vals = torch.randn((W, N), generator=g, device="cuda")
            a.step(acts, vals); b.step(acts, vals)
        if t % 10 == 9 or t < 5:
            _same(a.obs, b.obs, ("obs", t))
            for x, y in zip(ea.get_state(), eb.get_state()):
                _same(x, y, ("state", t))
            for name in ("rewards", "done", "game_over", "episode"):
                _same(getattr(ea, name), getattr(eb, name), (name, t))
            for name in ("x", "val", "ret", "act_ring", "emit_t", "dup_count"):
                _same(getattr(a, name), getattr(b, name), (name, t))
    ba, bb = a.drain(flush_all=True), b.drain(flush_all=True)
    assert len(ba) == len(bb) > 0 and ba.dropped == bb.dropped == 0
    if time_max > 5:
        rs.require_deep_flushes(bb.src.cpu().numpy(), time_max, "step_push N=%d W=%d reflush=%s" % (N, W, reflush))
    tw.compare_drained(ba, bb, ("step_push", N, W, reflush))
    epa, epb = a.drain_episodes().cpu().numpy(), b.drain_episodes().cpu().numpy()
    assert len(epa) == len(epb) > 0
    tw.compare_episode_records(epa, epb, ("step_push", N, W, reflush))
    for e, r in rolls:
        r.close(); e.close()


def test_rows_that_need_no_action_get_none():
    """The fused kernel runs the network only for the rows that still need an action (cavoid_actor.hpp, policy_split_tile<P, NRT>): right after a
    reset that is every learning agent -- scripted and absent agents' rows are handed action 0 / value 0 -- and a live row's value is bit for bit
    the stand-alone pass's on the same observation, whatever tile row the compaction moved it to."""
    env, net, pol, roll = _make(700, 4, 5, False, gen_min_agents=2, gen_nonlearning_fraction=0.5, gen_static_fraction=0.5)
    obs0 = roll.obs.clone()
    need = (obs0[..., 0] > 0.5)
    assert 0.2 < need.float().mean().item() < 0.8                       # a real mix: most tiles run 2 or 3 of their 4 row tiles
    roll.run_fused(1)
    torch.cuda.synchronize()
    acts, vals = roll._act_out.view(700, 4), roll._val_out.view(700, 4)      # (the kernel's hand-over buffers: the last step's actions / values)
    assert (acts[~need] == 0).all() and (vals[~need] == 0).all()
    _, v_ref = pol(obs0[..., 1:].reshape(700 * 4, -1))                   # the stand-alone kernel on every row
    assert torch.equal(vals[need], v_ref.view(700, 4)[need])
    assert (acts[need] >= 0).all() and (acts[need] < env.num_actions).all() and acts[need].float().std().item() > 0


def test_a_masked_reset_between_two_fused_launches_needs_no_flag_fixup():
    """done / game_over are OUTPUTS of cavoid_actor_run (include/cavoid.h): which rows need an action at a launch's first step is derived
    from the world state, not from what the previous launch left in those buffers.  A masked cavoid_reset between two launches leaves them
    stale for the reset worlds (done = 1 of an agent whose world now starts a new episode, game_over = 0): launch 2 must give those agents real
    actions all the same -- identical to a twin whose buffers were patched by hand to what round 5's kernel wanted to see."""
    W, N, seed, K1 = 2048, 4, 9, 40                          # (K1 even: the current observation is back in env.obs)
    env_a, _, _, a = _make(W, N, seed, False)
    env_b, _, _, b = _make(W, N, seed, False)
    for r in (a, b):
        r.run_fused(K1)
    _same(a.obs, b.obs, "after launch 1")
    # worlds that are NOT over but hold a finished learning agent: stale done = 1 after the reset
    stale = (env_a.done.bool() & (a.obs[..., 0] > 0.5)).any(dim=1) & (env_a.game_over == 0)
    assert int(stale.sum()) >= 5
    mask = stale.to(torch.uint8)
    for env in (env_a, env_b):
        env.reset(mask)                                      # writes the observation of all worlds into env.obs == the rollout's current buffer
    env_b.done[stale] = 0                                    # the twin: buffers as a step that restarted those worlds would have left them
    env_b.game_over[stale] = 1
    assert not torch.equal(env_a.done, env_b.done)
    for r in (a, b):
        r.run_fused(6)
    _same(a.obs, b.obs, "obs after launch 2")
    for x, y in zip(env_a.get_state(), env_b.get_state()):
        _same(x, y, "state after launch 2")
    for name in ("x", "val", "ret", "act_ring", "emit_t"):
        _same(getattr(a, name), getattr(b, name), name)
    # and the reset worlds' learning agents did act: their first step's ring entry is not the 'no action needed' filler everywhere
    t0 = K1 % a.ring_len
    acted = a.act_ring[t0].view(W, N)[stale]
    assert int((acted != 0).sum()) > 0
    for r in (a, b):
        r.close()
    env_a.close(); env_b.close()
