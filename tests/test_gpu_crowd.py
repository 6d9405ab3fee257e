"""The crowd step form (CAVOID_FORM_CROWD: worlds of 17..64 agents, one lane per agent, keys and ranks in LDS) on the GPU.

Against the float64 oracle at the bar of tests/test_gpu_parity.py (flags and float32 state bit-exact, float64 state <= 1e-9, obs and
rewards <= 1e-5, heading on the circle); its own launch forms against each other bitwise; and -- the drift guard on the copies of
env_tile's statements -- a development build that routes EVERY agent count to the crowd form, held bitwise to the product's tile
forms at N = 4 and 10."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import c_oracle as co
from tests.gpu_support import OBS_TOL, _compare_step, _env, _goal_seeking_actions, _pull, _push

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROWD = ("CROWD", 0)


def _gen(N, gen_min, nonl, box, pool=0):
    return co.default_gen(gen_min, N, nonl, 0.5, pool_size=pool, mode=1 if box else 0)


def _terminal_flags_seen(st):
    return (st.flags & 4 != 0).any() and (st.flags & 1 != 0).any() and (st.flags & 2 != 0).any()


@pytest.mark.parametrize("N,M,sort,nonl,gen_min,box", [
    (17, None, 0, 0.0, 17, True),
    (20, 7, 1, 0.3, 10, True),       # clipping, closest_first, scripted agents
    (20, 30, 0, 0.2, 12, False),     # M > N-1: padded slots; GEN v1 rings
    (32, None, 2, 0.0, 24, True),    # time-to-impact order
    (33, 19, 0, 0.3, 30, True),      # one world per wavefront
    (48, None, 1, 0.0, 40, True),
    (64, None, 0, 0.2, 50, True),
])
def test_crowd_trajectory_parity(N, M, sort, nonl, gen_min, box):
    W, steps, seed = 257, 120, 13
    ocfg = co.default_cfg(N, N - 1 if M is None else M, sort_method=sort)
    ogen = _gen(N, gen_min, nonl, box)
    env = _env(W, N, M, seed=seed, sort_method=sort, gen_min_agents=gen_min, gen_nonlearning_fraction=nonl, gen_mode=1 if box else 0,
               gen_pool_size=0)
    st = co.State.empty(W, N)
    co.generate(ocfg, ogen, seed, st, np.zeros(W, np.uint32))
    _push(env, st)
    np.testing.assert_allclose(env.observe().cpu().numpy(), co.observe(ocfg, st), rtol=0, atol=OBS_TOL)
    rng = np.random.default_rng(seed)
    for t in range(steps):
        acts = _goal_seeking_actions(rng, W, N)
        out = env.step(torch.from_numpy(acts).cuda())
        assert env.last_step_form == CROWD
        _compare_step(("crowd", N, M, sort, t), out, co.step(ocfg, st, acts), env, st)
    assert _terminal_flags_seen(st)                            # collisions, goals and time-outs all happen
    env.close()


@pytest.mark.parametrize("N,pool,box,nonl", [(20, 300, False, 0.2), (33, 0, True, 0.3), (64, 0, False, 0.0), (24, 200, True, 0.0)])
def test_crowd_autoreset_parity(N, pool, box, nonl):
    """restarts from the scenario pool (filled by the crowd form's reset) and from the generator inside the step, episode counters"""
    W, steps, seed = 129, 160, 5
    ocfg = co.default_cfg(N, N - 1)
    ogen = _gen(N, 2, nonl, box, pool)
    env = _env(W, N, seed=seed, gen_min_agents=2, gen_nonlearning_fraction=nonl, gen_mode=1 if box else 0, gen_pool_size=pool)
    obs0 = env.reset().cpu().numpy()
    st = co.State.empty(W, N)
    ep = np.zeros(W, np.uint32)
    co.generate(ocfg, ogen, seed, st, ep)
    f64, f32, fl = _pull(env)
    assert np.array_equal(fl, st.flags) and np.array_equal(f32, st.f32)
    np.testing.assert_allclose(obs0, co.observe(ocfg, st), rtol=0, atol=OBS_TOL)
    rng = np.random.default_rng(seed)
    for t in range(steps):
        acts = _goal_seeking_actions(rng, W, N)
        out = env.step_autoreset(torch.from_numpy(acts).cuda())
        assert env.last_step_form == CROWD
        _compare_step(("crowd-auto", N, pool, t), out, co.step_autoreset(ocfg, ogen, seed, st, ep, acts), env, st)
        assert np.array_equal(env.episode.cpu().numpy().view(np.uint32), ep)
    assert ep.max() >= 1
    K = 20                                                     # the in-launch step loop, every step's outputs in its slot
    acts = np.stack([_goal_seeking_actions(rng, W, N) for _ in range(K)])
    obs, rew, done, go = env.step_autoreset_n(torch.from_numpy(acts).cuda(), slots=env.new_step_slots(K))
    assert env.last_step_form == CROWD
    for t in range(K):
        oobs, orew, odone, ogo = co.step_autoreset(ocfg, ogen, seed, st, ep, acts[t])
        assert np.array_equal(done[t].cpu().numpy(), odone) and np.array_equal(go[t].cpu().numpy(), ogo), t
        d = np.abs(obs[t].cpu().numpy() - oobs)
        d[..., 3] = np.minimum(d[..., 3], np.abs(d[..., 3] - 2 * np.pi))
        assert d.max() <= OBS_TOL and np.abs(rew[t].cpu().numpy() - orew).max() <= OBS_TOL, t
    assert np.array_equal(_pull(env)[2], st.flags) and np.array_equal(env.episode.cpu().numpy().view(np.uint32), ep)
    env.close()


def _pair(N, W, seed, **over):
    a, b = _env(W, N, seed=seed, **over), _env(W, N, seed=seed, **over)
    a.reset(); b.reset()
    return a, b


def _same_state(a, b):
    for x, y in zip(a.get_state(), b.get_state()):
        assert torch.equal(x, y)
    assert torch.equal(a.episode, b.episode)


@pytest.mark.parametrize("N,dyn", [(20, 0), (40, 1)])
def test_crowd_k_step_launches_equal_single_steps(N, dyn):
    """step_autoreset_n of K steps == K one-step launches, bitwise: slots, stride 0, packed, out-of-range actions"""
    W, seed = 97, 7
    a, b = _pair(N, W, seed, gen_pool_size=300, gen_nonlearning_fraction=0.3, dynamics=dyn)
    rng = np.random.default_rng(seed)
    for K in (1, 2, 17, 64, 129):
        acts = torch.from_numpy(rng.integers(-2, 14, size=(K, W, N)).astype(np.int32)).cuda()    # (clamped to the table)
        slots = a.new_step_slots(K)
        obs, rew, done, go = a.step_autoreset_n(acts, slots=slots)
        assert a.last_step_form == CROWD
        for t in range(K):
            o, r, d, g = b.step_autoreset(acts[t])
            assert torch.equal(obs[t], o) and torch.equal(rew[t], r) and torch.equal(done[t], d) and torch.equal(go[t], g), (K, t)
        _same_state(a, b)
    acts = torch.from_numpy(rng.integers(0, 11, size=(9, W, N)).astype(np.int32)).cuda()
    a.step_autoreset_n(acts)                                   # stride 0: every step overwrites slot 0
    for t in range(9):
        b.step_autoreset(acts[t])
    assert torch.equal(a.obs, b.obs) and torch.equal(a.rewards, b.rewards) and torch.equal(a.done, b.done)
    _same_state(a, b)
    pk = a.new_step_slots(5, packed=True)                      # packed records == the plain outputs
    acts = torch.from_numpy(rng.integers(0, 11, size=(5, W, N)).astype(np.int32)).cuda()
    pk_all, go_all = a.step_autoreset_packed(acts, pk)
    wdt = a.obs_width
    for t in range(5):
        o, r, d, g = b.step_autoreset(acts[t])
        p = pk_all[t]
        assert torch.equal(p[..., :wdt], o) and torch.equal(p[..., wdt], r) and torch.equal(p[..., wdt + 1], d.float()), t
        assert torch.equal(go_all[t], g)
    _same_state(a, b)
    a.close(); b.close()


def _padded_k_step(env, acts, pad, cont=False):
    """one K-step launch whose action slices lie pad elements (int32 / float) apart beyond their own size, every step in its slot"""
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    K = acts.shape[0]
    flat = acts.reshape(K, -1)
    buf = torch.full((K, flat.shape[1] + pad), 99, dtype=flat.dtype, device=flat.device)    # (what lies in the padding is never read)
    buf[:, :flat.shape[1]] = flat
    slots = env.new_step_slots(K)
    p = BatchedCollisionAvoidanceEnv._ptr
    fn = env._lib.cavoid_step_continuous_autoreset_n if cont else env._lib.cavoid_step_autoreset_n
    _lib.check(fn(env._h, p(buf), buf.shape[1], K, env.num_worlds, p(slots.obs), p(slots.rewards), p(slots.done), p(slots.game_over),
                  env._stream()), "padded K-step launch")
    return slots.obs, slots.rewards, slots.done, slots.game_over


def test_crowd_k_step_with_padded_action_strides():
    N, W, seed, K = 28, 45, 11, 19
    a, b = _pair(N, W, seed, gen_pool_size=150, gen_nonlearning_fraction=0.2)
    rng = np.random.default_rng(seed)
    acts = torch.from_numpy(rng.integers(-3, 15, size=(K, W, N)).astype(np.int32)).cuda()
    obs, rew, done, go = _padded_k_step(a, acts, 37)
    assert a.last_step_form == CROWD
    for t in range(K):
        o, r, d, g = b.step_autoreset(acts[t])
        assert torch.equal(obs[t], o) and torch.equal(rew[t], r) and torch.equal(done[t], d) and torch.equal(go[t], g), t
    _same_state(a, b)
    cacts = torch.from_numpy(rng.uniform(-1.5, 1.5, size=(K, W, N, 2)).astype(np.float32)).cuda()
    obs, rew, done, go = _padded_k_step(a, cacts, 10, cont=True)
    for t in range(K):
        o, r, d, g = b.step_continuous_autoreset(cacts[t])
        assert torch.equal(obs[t], o) and torch.equal(rew[t], r) and torch.equal(done[t], d) and torch.equal(go[t], g), t
    _same_state(a, b)
    a.close(); b.close()


@pytest.mark.parametrize("dyn", [0, 2])
def test_crowd_continuous_k_step_equals_single_steps(dyn):
    N, W, seed, K = 24, 65, 9, 12
    a, b = _pair(N, W, seed, gen_pool_size=200, dynamics=dyn)
    rng = np.random.default_rng(seed)
    acts = torch.from_numpy(rng.uniform(-1.5, 1.5, size=(K, W, N, 2)).astype(np.float32)).cuda()
    slots = a.new_step_slots(K)
    obs, rew, done, go = a.step_continuous_autoreset(acts, slots=slots)
    assert a.last_step_form == CROWD
    for t in range(K):
        o, r, d, g = b.step_continuous_autoreset(acts[t])
        assert torch.equal(obs[t], o) and torch.equal(rew[t], r) and torch.equal(done[t], d) and torch.equal(go[t], g), t
    _same_state(a, b)
    a.close(); b.close()


def test_crowd_packed_reset_observe_and_state_roundtrips():
    N, W, seed = 36, 50, 3
    env = _env(W, N, seed=seed, gen_pool_size=100, gen_min_agents=20)
    obs = env.reset().clone()
    pk = env.reset_packed(env.new_packed())                   # (a reset starts the NEXT episode: compare on a twin)
    twin = _env(W, N, seed=seed, gen_pool_size=100, gen_min_agents=20)
    twin.reset()
    o2 = twin.reset().clone()
    assert torch.equal(pk[..., :env.obs_width], o2)
    assert torch.equal(env.observe(), o2) and torch.equal(env.observe_packed(env.new_packed())[..., :env.obs_width], o2)
    mask = torch.from_numpy((np.arange(W) % 3 == 0).astype(np.uint8)).cuda()
    ep_before = env.episode.clone()
    env.reset(mask)
    assert torch.equal(env.episode - ep_before, mask.to(env.episode.dtype))
    sd = env.state_dict()
    acts = torch.from_numpy(np.random.default_rng(1).integers(0, 11, size=(W, N)).astype(np.int32)).cuda()
    o_a = env.step_autoreset(acts)[0].clone()
    twin.load_state_dict(sd)
    o_b = twin.step_autoreset(acts)[0]
    assert torch.equal(o_a, o_b)
    _same_state(env, twin)
    f64, f32, fl = env.get_state()
    twin.set_state(f64, f32, fl)
    assert torch.equal(twin.observe(), env.observe())
    del obs
    env.close(); twin.close()


@pytest.mark.parametrize("over", [dict(wrap_closed_end=1, done_agents_collide=0, sort_round_gap=0, sort_tie_lateral=0),
                                  dict(done_agents_collide=0), dict(sort_tie_lateral=0),
                                  dict(close_penalty_slope=-0.5, actions_fp32=0, timeout_enabled=0, time_budget_from_goal_edge=0),
                                  dict(sensing_horizon=3.0), dict(evaluate_mode=1)])
def test_crowd_switches_follow_the_oracle(over):
    N, W, steps, seed = 21, 129, 80, 8
    ocfg = co.default_cfg(N, N - 1, **over)
    ogen = _gen(N, 10, 0.3, True)
    env = _env(W, N, seed=seed, gen_min_agents=10, gen_nonlearning_fraction=0.3, gen_mode=1, gen_pool_size=0, **over)
    env.reset()
    st = co.State.empty(W, N)
    ep = np.zeros(W, np.uint32)
    co.generate(ocfg, ogen, seed, st, ep)
    _push(env, st)
    rng = np.random.default_rng(seed)
    for t in range(steps):
        acts = _goal_seeking_actions(rng, W, N)
        out = env.step_autoreset(torch.from_numpy(acts).cuda())
        _compare_step(("crowd-U", over, t), out, co.step_autoreset(ocfg, ogen, seed, st, ep, acts), env, st)
    env.close()


@pytest.mark.parametrize("sort", [0, 1, 2])
def test_crowd_exact_ties_take_the_generic_rank_path(sort):
    """tests/test_gpu_parity.py's mirrored pair, in a world of 20 (the other 16 agents absent): equal keys, the exact rule.
    (Ties of three, inside the M cut, of the float32 lateral alone, of the exact-gap keys, over the steps of one launch, and the threshold
    predicates at equality, through every launch form of 17, 33 and 64 agents: tests/tie_regimes.py, tests/test_gpu_tie_regimes.py.)"""
    W, N = 40, 20
    ocfg = co.default_cfg(N, N - 1, sort_method=sort)
    env = _env(W, N, sort_method=sort)
    st = co.State.empty(W, N)
    rng = np.random.default_rng(4)
    for w in range(W):
        k = slice(w * N, w * N + 4)
        if w % 2 == 0:
            st.f64[0, k] = [0.0, 1.0, -1.0, 0.0]
            st.f64[1, k] = [0.0, 0.8, 0.8, -2.0]
            st.f32[0, k] = [5.0, 1.0, -1.0, 0.0]
            st.f32[1, k] = [0.0, 5.0, 5.0, -6.0]
            st.f32[2, k] = 0.3
        else:
            st.f64[0, k] = rng.uniform(-4, 4, 4)
            st.f64[1, k] = rng.uniform(-4, 4, 4)
            st.f32[0, k] = rng.uniform(-6, 6, 4)
            st.f32[1, k] = rng.uniform(-6, 6, 4)
            st.f32[2, k] = rng.uniform(0.2, 0.5, 4)
        st.f32[3, k] = 1.0
        st.f64[2, k] = np.arctan2(st.f32[1, k] - st.f64[1, k], st.f32[0, k] - st.f64[0, k])
        st.f64[3, k] = 50.0
        st.flags[k] = 0x20 | 0x40
    _push(env, st)
    want = co.observe(ocfg, st)
    np.testing.assert_allclose(env.observe().cpu().numpy(), want, rtol=0, atol=OBS_TOL)
    gaps = want[0, 0][6 + 6::7][:3]
    assert np.min(np.abs(np.subtract.outer(gaps, gaps))[~np.eye(3, dtype=bool)]) < 1e-12
    for t in range(5):
        acts = np.full((W, N), 2, np.int32)
        _compare_step(("crowd-ties", sort, t), env.step(torch.from_numpy(acts).cuda()), co.step(ocfg, st, acts), env, st)
    env.close()


def test_crowd_refusals_are_errors():
    from rl_collision_avoidance_amd import _lib
    with pytest.raises(_lib.CavoidError):
        _env(8, 20, rvo_enabled=1)
    with pytest.raises(_lib.CavoidError):
        _env(8, 20, gen_pool_size=0, gen_lookahead=8)
    with pytest.raises(_lib.CavoidError):
        _env(8, 65, 19)


def _rollout_rows(N, fused_policy):
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    env = _env(64, N, seed=2, gen_pool_size=0, gen_min_agents=2)
    net = NetworkVP_rnn(env.config).to("cuda:0")
    pol = FusedPolicy(net, seed=3) if fused_policy else net.predict_p_and_v
    roll = BatchedRollout(env, pol, time_max=3)
    assert not roll.fused_available and "more than 16 agents" in roll.fused_unavailable_reason
    roll.reset()
    for _ in range(12):
        roll.step()
    assert env.last_step_form == CROWD
    batch = roll.drain()
    rows = int(batch.x.shape[0])
    assert batch.x.shape[1] == env.obs_width - 1 and torch.isfinite(batch.x).all() and torch.isfinite(batch.r).all()
    roll.close(); env.close()
    return rows


def test_crowd_rollout_with_the_fused_policy_and_the_torch_network():
    assert _rollout_rows(20, True) > 0        # M = 19: the fused policy kernel, the env step + cavoid_rollout_push
    assert _rollout_rows(32, False) > 0       # M = 31: the PyTorch network


# ---- drift guard: the crowd kernel's copies of env_tile's statements --------------------------------------------------------------
_DRIFT_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[2])
from tests.gpu_support import _env
# (tag, M offset from N - 1, overrides): the default configuration; closest_first with GEN v2 generated inside the step, the max-turn-rate
# dynamics and U2 / U4 / U7b flipped; time-to-impact with exact gaps, a finite horizon, clipping, evaluate mode and the U1 / U5 / U11
# switches; holonomic dynamics (continuous actions only)
CONFIGS = [
    ("default", 0, dict(gen_pool_size=500, gen_nonlearning_fraction=0.3, gen_min_agents=2)),
    ("box", 0, dict(sort_method=1, gen_mode=1, gen_pool_size=0, dynamics=1, gen_nonlearning_fraction=0.4, gen_min_agents=2,
                    wrap_closed_end=1, done_agents_collide=0, sort_tie_lateral=0)),
    ("tti", -1, dict(sort_method=2, sort_round_gap=0, sensing_horizon=3.0, evaluate_mode=1, gen_pool_size=300, gen_nonlearning_fraction=0.3,
                     gen_min_agents=2, close_penalty_slope=-0.5, actions_fp32=0, timeout_enabled=0, time_budget_from_goal_edge=0)),
    ("holo", 0, dict(dynamics=2, gen_pool_size=200, gen_min_agents=2)),
]
out = {}
for tag, dm, over in CONFIGS:
    for N in (4, 10):
        W, seed = 300, 21
        key = lambda name: "%s_%s%d" % (tag, name, N)
        rng = np.random.default_rng(N)
        e = _env(W, N, N - 1 + dm, seed=seed, **over)
        table = over.get("dynamics", 0) != 2
        out[key("reset")] = e.reset().cpu().numpy()
        out[key("observe")] = e.observe().cpu().numpy()
        if table:
            a = torch.from_numpy(rng.integers(-1, 12, size=(W, N)).astype(np.int32)).cuda()
            o, r, d, g = e.step(a)
            out[key("step")] = np.concatenate([o.cpu().numpy().ravel(), r.cpu().numpy().ravel(), d.cpu().numpy().ravel(), g.cpu().numpy().ravel()])
            for t in range(3):
                o, r, d, g = e.step_autoreset(torch.from_numpy(rng.integers(0, 11, size=(W, N)).astype(np.int32)).cuda())
                out[key("auto%d_" % t)] = np.concatenate([o.cpu().numpy().ravel(), r.cpu().numpy().ravel(), d.cpu().numpy().ravel()])
            K = 17
            o, r, d, g = e.step_autoreset_n(torch.from_numpy(rng.integers(0, 11, size=(K, W, N)).astype(np.int32)).cuda(), slots=e.new_step_slots(K))
            out[key("kstep")] = np.concatenate([o.cpu().numpy().ravel(), r.cpu().numpy().ravel(), d.cpu().numpy().ravel(), g.cpu().numpy().ravel()])
            pk, go = e.step_autoreset_packed(torch.from_numpy(rng.integers(0, 11, size=(5, W, N)).astype(np.int32)).cuda(), e.new_step_slots(5, packed=True))
            out[key("packed")] = pk.cpu().numpy()
        c = torch.from_numpy(rng.uniform(-1, 1, size=(4, W, N, 2)).astype(np.float32)).cuda()
        o, r, d, g = e.step_continuous_autoreset(c, slots=e.new_step_slots(4))
        out[key("cont")] = np.concatenate([o.cpu().numpy().ravel(), r.cpu().numpy().ravel(), d.cpu().numpy().ravel(), g.cpu().numpy().ravel()])
        o, r, d, g = e.step_continuous_autoreset(c[0])
        out[key("cont1")] = np.concatenate([o.cpu().numpy().ravel(), r.cpu().numpy().ravel(), d.cpu().numpy().ravel(), g.cpu().numpy().ravel()])
        out[key("mreset")] = e.reset(torch.from_numpy((np.arange(W) % 2).astype(np.uint8)).cuda()).cpu().numpy()
        f64, f32, fl = e.get_state()
        out[key("state")] = np.concatenate([f64.cpu().numpy().view(np.uint8).ravel(), f32.cpu().numpy().view(np.uint8).ravel(),
                                            fl.cpu().numpy().view(np.uint8).ravel(), e.episode.cpu().numpy().view(np.uint8).ravel()])
        out[key("form")] = np.array([ord(ch) for ch in e.last_step_form[0]])
        e.close()
np.savez(sys.argv[1], **out)
"""


def _drift_run(tmp_path, tag, lib):
    path = str(tmp_path / ("%s.npz" % tag))
    env = dict(os.environ)
    if lib:
        env["CAVOID_LIB"] = lib
    else:
        env.pop("CAVOID_LIB", None)
    subprocess.run([sys.executable, "-c", _DRIFT_CHILD, path, ROOT], env=env, check=True, timeout=600)
    return dict(np.load(path))


def test_crowd_form_equals_the_tile_forms_bitwise_at_small_n(tmp_path):
    from rl_collision_avoidance_amd import build
    variant = build.variant_path("crowd2")
    if not os.path.exists(variant):
        try:
            build.hipcc()
        except RuntimeError:
            pytest.skip("no prebuilt crowd development variant and no hipcc to build it")
        variant = build.build_crowd_dev()
    tile = _drift_run(tmp_path, "tile", None)
    crowd = _drift_run(tmp_path, "crowd", variant)
    assert sorted(tile) == sorted(crowd)
    for k in tile:
        if "_form" in k:
            assert "".join(map(chr, crowd[k])) == "CROWD" and "".join(map(chr, tile[k])) != "CROWD", k
            continue
        assert tile[k].shape == crowd[k].shape, k
        assert np.array_equal(tile[k].view(np.uint8), crowd[k].view(np.uint8)), k
