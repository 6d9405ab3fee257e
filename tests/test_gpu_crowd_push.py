"""`cavoid_step_push` on crowd worlds (17..64 agents per world): `crowd_push_kernel` (csrc/cavoid_crowd_push.hpp) -- one auto-reset
step of every world, that step's Experience bookkeeping and the episode log in ONE launch, one workgroup of two wavefronts per tile
(env step + bookkeeping on one, the copy of the step's state rows on the other).

Held bitwise to the three launches it replaces (`crowd_kernel`, `rollout_push_kernel`, `rollout_episode_kernel`: the code of before,
untouched), to the pinned rollout oracle, through the C ABI's refusals, and through a hipGraph with the device-side step counter."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import rollout_oracle as ro
from tests import rollout_scripts as rs
from tests.gpu_support import _env

pytestmark = pytest.mark.gpu

CROWD = ("CROWD", 0)
ONE, THREE = "step_push", "env, push, episode log"
R_TOL = 1e-6      # n-step returns: float64 on both sides, emitted as float32 (tests/test_gpu_rollout.py)


def _same(a, b, what):
    assert torch.equal(a, b), what


def _rollout(env, reflush, steps, fuse, **kw):
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    # room for every duplicate row of the re-flush quirk (at most one per slot and step): a full buffer drops rows in arrival order, which
    # legitimately differs between the forms
    roll = BatchedRollout(env, None, reflush_done=reflush, dup_capacity=env.num_worlds * env.max_agents * steps if reflush else None,
                          **kw)
    roll.fuse_env_push = fuse
    roll.reset()
    return roll


# (N, W, M, reflush, settings): the lane mappings of the crowd form -- three / two / one world per wavefront, idle lanes, a ragged last
# wavefront, all 64 lanes, the full-width world mask -- with absent agents and learning counts below N (gen_min_agents=2 + a non-learning
# fraction), restarts from the pool and from the generator inside the step, M < N - 1.
# steps, straight: the step count, and how many of the first worlds are scripted 'full speed straight ahead' only.  Worlds that start
# with 2..N agents (gen_min_agents=2) finish within 150 steps of the biased random actions.  The N = 32 case keeps all 32 agents of
# every world present and learning, and a world ends only when its last agent has: one random turn makes an agent miss its goal and
# run until its time-out (2 x its straight-line time), 500 to 700 steps in.  Its first 10 worlds therefore go straight only -- every
# agent reaches its goal or collides, the first of them ends about 200 steps in and half a dozen have ended and restarted from the pool
# after 280 -- while the other 30 worlds keep the random mix.  The N = 64 case draws 9 to 61 agents per world; of its 12 worlds only the
# 9-agent one ends within 400 steps of the random mix, and when depends on the mix.  Its first 6 worlds go straight only: the 15- and
# 16-agent worlds among them end about 120, 145 and 190 steps in.
@pytest.mark.parametrize("N,W,M,reflush,over,steps,straight", [
    (17, 50, 16, True, dict(gen_min_agents=2, gen_nonlearning_fraction=0.3), 150, 0),
    (22, 33, 21, False, dict(gen_mode=1, gen_pool_size=0, gen_min_agents=2), 150, 0),
    (32, 40, 31, True, dict(gen_pool_size=200), 280, 10),
    (33, 20, 19, False, dict(gen_min_agents=2), 150, 0),
    (64, 12, 63, True, dict(gen_min_agents=2, gen_nonlearning_fraction=0.2), 200, 6),
    # the backward pass past its 32 registers (time_max + 1 > 32: the serial form) and with all 32 live, on a ring of 2 time_max + 12 blocks
    (20, 24, 19, True, dict(time_max=33, gen_min_agents=2, gen_nonlearning_fraction=0.3), 150, 0),
    (20, 24, 19, False, dict(time_max=33, gen_min_agents=2), 150, 0),
    (20, 24, 19, False, dict(time_max=31, gen_min_agents=2), 150, 0),
])
def test_crowd_step_push_equals_step_then_push(N, W, M, reflush, over, steps, straight):
    """One launch against the three it replaces, bitwise, with scripted actions / values from one generator; time_max = 5 and a ring
    of 12 blocks that wraps a dozen times and more (the time_max = 33 / 31 cases: a ring of 2 time_max + 12 blocks that wraps once).  Actions are biased to 'full speed straight ahead' so that agents reach goals
    and worlds finish (tests/test_gpu_parity.py's _goal_seeking_actions)."""
    over = dict(over)
    time_max = over.pop("time_max", 5)
    STEPS, RING = steps, 12 if time_max == 5 else 2 * time_max + 12
    rolls = []
    for fuse in (True, False):
        env = _env(W, N, M, seed=17, **over)
        rolls.append((env, _rollout(env, reflush, STEPS, fuse, time_max=time_max, ring_len=RING)))
    (ea, a), (eb, b) = rolls
    assert a.step_path == ONE and b.step_path == THREE
    g = torch.Generator(device="cuda").manual_seed(3)
    emitted_b = 0
    for t in range(STEPS):
        acts = torch.randint(0, 11, (W, N), generator=g, device="cuda", dtype=torch.int32)
        acts[torch.rand((W, N), generator=g, device="cuda") < 0.8] = 2
        acts[:straight] = 2
        vals = torch.randn((W, N), generator=g, device="cuda")
        a.step(acts, vals); b.step(acts, vals)
        if t == 0:
            assert ea.last_step_form == CROWD and eb.last_step_form == CROWD
        if t % 10 == 9 or t < 5:
            _same(a.obs, b.obs, ("obs", t))
            for x, y in zip(ea.get_state(), eb.get_state()):
                _same(x, y, ("state", t))
            for name in ("rewards", "done", "game_over", "episode"):
                _same(getattr(ea, name), getattr(eb, name), (name, t))
            for name in ("x", "val", "ret", "act_ring", "emit_t", "dup_count"):
                _same(getattr(a, name), getattr(b, name), (name, t))
            emitted_b = max(emitted_b, int((b.emit_t >= 0).sum().item()))
    dup_b = b.dup_count.tolist()
    ba, bb = a.drain(flush_all=True), b.drain(flush_all=True)
    epa, epb = a.drain_episodes().cpu().numpy(), b.drain_episodes().cpu().numpy()
    print("crowd step_push N=%d W=%d: three-launch side emitted %d ring rows at most, drained %d rows, %d duplicates (%d dropped), %d episodes"
          % (N, W, emitted_b, len(bb), dup_b[0], dup_b[1], len(epb)))
    # the three-launch side (the code of before) did what the case is about: nothing below passes on nothing
    assert emitted_b > 0 and len(bb) > 0 and len(epb) > 0
    assert dup_b[1] == 0 and (dup_b[0] > 0 if reflush else dup_b[0] == 0)
    if time_max > 5:
        rs.require_deep_flushes(bb.src.cpu().numpy(), time_max, "crowd step_push N=%d W=%d reflush=%s" % (N, W, reflush))
    assert len(ba) == len(bb) and ba.dropped == bb.dropped == 0
    ka, kb = np.lexsort(ba.src.cpu().numpy().T[::-1]), np.lexsort(bb.src.cpu().numpy().T[::-1])
    for name in ("src", "x", "r", "a_index"):
        assert np.array_equal(getattr(ba, name).cpu().numpy()[ka], getattr(bb, name).cpu().numpy()[kb]), name
    assert len(epa) == len(epb)
    epa, epb = epa[np.lexsort(epa.T[::-1])], epb[np.lexsort(epb.T[::-1])]
    assert np.array_equal(epa[:, 0], epb[:, 0]) and np.array_equal(epa[:, 2], epb[:, 2])
    np.testing.assert_allclose(epa[:, 1], epb[:, 1], rtol=1e-6, atol=1e-6)       # (double atomics whose order varies)
    for e, r in rolls:
        r.close(); e.close()


@pytest.mark.parametrize("reflush,T_MAX", [pytest.param(True, 20, id="True"), pytest.param(False, 20, id="False"),
                                            pytest.param(True, 33, id="True-tmax33")])       # 33: the serial backward pass
def test_crowd_step_push_matches_the_rollout_oracle(reflush, T_MAX):
    """The one-launch path on a crowd env against oracle/rollout_oracle.run_episode, world by world and episode by episode, the way
    tests/test_gpu_rollout.py::test_rollout_matches_oracle holds the tile forms: rows and actions exact, returns to R_TOL, episode
    lengths exact, episode totals to its atol = 1e-4."""
    N, W, steps, seed, GAMMA = 20, 24, 160, 3, 0.97
    env = _env(W, N, seed=seed, gen_min_agents=2, gen_nonlearning_fraction=0.3)
    roll = _rollout(env, reflush, steps, True, time_max=T_MAX, discount=GAMMA, ring_len=steps + 8)
    assert roll.step_path == ONE
    rng = np.random.default_rng(seed)
    rec = []
    for t in range(steps):
        obs = roll.obs.cpu().numpy().copy()
        acts = rng.integers(0, 11, size=(W, N)).astype(np.int32)
        acts[rng.random((W, N)) < 0.7] = 2
        vals = np.round(rng.normal(0, 0.5, size=(W, N)), 3).astype(np.float32)
        rew, done, over = roll.step(torch.from_numpy(acts).cuda(), torch.from_numpy(vals).cuda())
        rec.append((obs, acts, vals, rew.cpu().numpy().copy(), done.cpu().numpy().astype(bool), over.cpu().numpy().astype(bool)))
    assert env.last_step_form == CROWD
    batch = roll.drain(flush_all=True)
    episodes = roll.drain_episodes().cpu().numpy()
    assert batch.dropped == 0 and len(batch) > 0
    x, r, a, src = [v.cpu().numpy() for v in (batch.x, batch.r, batch.a_index, batch.src)]
    if T_MAX > 20:
        rs.require_deep_flushes(src, T_MAX, "crowd step_push vs oracle")
    got = {}
    for k in range(len(r)):
        got.setdefault(tuple(src[k]), []).append(k)          # (world, agent, recorded-at, emitted-at)

    expect_rows, expect_eps = 0, []
    for w in range(W):
        start = 0
        for t in range(steps):
            if not rec[t][5][w]:
                continue
            ts = list(range(start, t + 1))
            obs_seq = np.stack([rec[k][0][w] for k in ts] + [rec[t][0][w]])   # last entry unused by the oracle
            learning = obs_seq[0][:, 0] > 0.5
            n_present = int(np.flatnonzero(obs_seq[0][:, 4] > 0).max()) + 1
            rewards = np.stack([rec[k][3][w] for k in ts]).astype(np.float64)
            done = np.stack([rec[k][4][w] for k in ts])
            actions = np.stack([rec[k][1][w] for k in ts])
            values = np.stack([rec[k][2][w] for k in ts]).astype(np.float64)
            chunks = ro.run_episode(obs_seq.astype(np.float64), rewards, done, learning, n_present, actions, values, GAMMA, T_MAX)
            if not reflush:          # cleaned mode: drop what a done-and-trained agent would re-flush
                trained_at, kept = {}, []
                for c in chunks:
                    if c.agent in trained_at and c.emitted_t > trained_at[c.agent]:
                        continue
                    kept.append(c)
                    if done[c.emitted_t, c.agent]:
                        trained_at.setdefault(c.agent, c.emitted_t)
                chunks = kept
            total_reward, total_length = 0.0, 0
            for c in chunks:
                emitted = start + c.emitted_t
                for row, tl in enumerate(c.t):
                    key = (w, c.agent, start + tl, emitted)
                    assert key in got and got[key], (key, "missing row")
                    k = got[key].pop(0)
                    assert np.array_equal(x[k], c.x[row].astype(np.float32)), key
                    assert abs(r[k] - c.r[row]) <= R_TOL, (key, r[k], c.r[row])
                    assert a[k] == int(np.argmax(c.a[row])), key
                    expect_rows += 1
                total_reward += c.score
                total_length += len(c.r) + 1
            if reflush:
                expect_eps.append((w, total_reward, total_length))
            start = t + 1
    print("crowd step_push vs oracle (reflush=%s): %d rows of finished episodes checked, %d device rows, %d episodes"
          % (reflush, expect_rows, len(r), len(episodes)))
    assert expect_rows > 0 and len(episodes) > 0
    leftover = sum(len(v) for v in got.values())
    assert expect_rows + leftover == len(r)
    finished_until = {w: max([t for t in range(steps) if rec[t][5][w]], default=-1) for w in range(W)}
    for key, ks in got.items():
        if ks:
            assert key[3] > finished_until[key[0]], ("unexpected row", key)
    if reflush:
        assert len(episodes) == len(expect_eps)
        dev = sorted((int(e[0]), round(float(e[2]))) for e in episodes)
        assert dev == sorted((w, tl) for w, _, tl in expect_eps)
        np.testing.assert_allclose(sorted(float(e[1]) for e in episodes), sorted(tr for _, tr, _ in expect_eps), atol=1e-4)
    roll.close()
    env.close()


def _step_push(env, roll, step=-1):
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    p = BatchedCollisionAvoidanceEnv._ptr
    W, N = env.num_worlds, env.max_agents
    acts = torch.full((W, N), 2, dtype=torch.int32, device="cuda")
    vals = torch.zeros((W, N), dtype=torch.float32, device="cuda")
    nxt = torch.zeros_like(env.obs)
    rc = env._lib.cavoid_step_push(env._h, roll._h, C.byref(roll._actor_buffers()), p(env.obs), p(nxt), p(acts), p(vals), p(env.rewards),
                                   p(env.done), p(env.game_over), step, env._stream())
    torch.cuda.synchronize()
    return rc, nxt


def test_crowd_step_push_c_abi():
    """cavoid_step_push carries a 20-agent env (CAVOID_OK, the crowd form reported); holonomic dynamics and a rollout handle made for
    another agent count are refused as before."""
    OK, EINVAL, EUNSUPPORTED = 0, -1, -4
    env = _env(24, 20, seed=5)
    roll = _rollout(env, False, 1, True, time_max=5)
    twin = _env(24, 20, seed=5)
    twin.reset()
    rc, nxt = _step_push(env, roll, step=0)
    assert rc == OK and env.last_step_form == CROWD
    acts = torch.full((24, 20), 2, dtype=torch.int32, device="cuda")
    assert torch.equal(nxt, twin.step_autoreset(acts)[0])              # ... and it is the step cavoid_step_autoreset takes
    assert torch.equal(env.rewards, twin.rewards) and torch.equal(env.done, twin.done)

    holo = _env(24, 20, seed=5, dynamics=2)
    roll_h = _rollout(holo, False, 1, True, time_max=5)
    assert roll_h.step_path == THREE
    assert _step_push(holo, roll_h)[0] == EUNSUPPORTED

    other = _env(24, 24, seed=5)
    roll_o = _rollout(other, False, 1, True, time_max=5)
    assert _step_push(env, roll_o)[0] == EINVAL
    for r in (roll, roll_h, roll_o):
        r.close()
    for e in (env, twin, holo, other):
        e.close()


def test_crowd_step_push_in_a_hipgraph_uses_the_device_side_step_counter():
    """capture(2) + replay(10) of the closed loop -- the crowd policy kernel (M = 23), then crowd_push_kernel with step < 0 and
    actor_finish_kernel advancing the counter -- against the same steps taken eagerly on a twin: the capture's 2 warm-up steps + the 20
    replayed ones = 22 step() calls.  Observations, env state, rings and step_index bitwise."""
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    N, W = 24, 32
    outs = []
    for graphed in (True, False):
        env = _env(W, N, seed=2, gen_min_agents=2, gen_nonlearning_fraction=0.2)
        torch.manual_seed(1234)
        net = NetworkVP_rnn(env.config).to("cuda:0")
        pol = FusedPolicy(net, seed=77)
        assert pol.max_others == N - 1
        roll = BatchedRollout(env, pol, reflush_done=False, time_max=5, ring_len=32)
        assert roll.step_path == ONE
        roll.reset()
        if graphed:
            roll.capture(2)
            roll.replay(10)
        else:
            for _ in range(2 + 20):
                roll.step()
        torch.cuda.synchronize()
        assert env.last_step_form == CROWD
        outs.append((roll.obs.clone(), [t.clone() for t in env.get_state()], env.episode.clone(),
                     [getattr(roll, n).clone() for n in ("x", "val", "ret", "act_ring", "emit_t")], roll.step_index))
        roll.close(); env.close()
    (o0, s0, e0, r0, n0), (o1, s1, e1, r1, n1) = outs
    assert n0 == n1 == 22
    assert torch.equal(o0, o1) and all(torch.equal(u, v) for u, v in zip(s0, s1)) and torch.equal(e0, e1)
    assert all(torch.equal(u, v) for u, v in zip(r0, r1))
    assert (r0[4] >= 0).any()                                       # rows were emitted
