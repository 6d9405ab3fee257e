"""GPU parity cases for `cavoid_cfg` fields the ABI exposes and the recorded configuration leaves at a neutral value:
a FINITE `sensing_horizon` (SENSING_HORIZON, run-ws/config.yaml:249-251 records inf -- the sensor drops every agent beyond
it, so the neighbour count, the clipping and the slot order all change) and a non-zero `reward_time_step` (REWARD_TIME_STEP,
:326-328 -- the reward every step starts from).  HIP vs the float64 oracle through EVERY form the env step is launched in:
one step per launch, the in-launch step loop as relay / two-wavefront pipeline / single wavefront with register prefetch /
plain loop, the N = 10 loop, and the packed-record outputs.

And EVERY numeric field off its default at once (tests/cfg_regimes.py: CLIPPED / UNCLIPPED beside the RING and BOX generator sets), through
the same forms; tests/test_cfg_regimes_host.py proves on the CPU that each field decides something within each case's steps."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import replay as rp
from oracle import c_oracle as co
from tests import cfg_regimes as R
from tests.cfg_regimes import WIDE          # turns beyond max_turn_rate * dt (0.6 rad), straight ahead at index 2: the max-turn clamp really acts

pytestmark = pytest.mark.gpu

OBS_TOL, STATE_TOL = 1e-5, 1e-9
FIELDS = dict(sensing_horizon=3.0, reward_time_step=-0.01)

def _env(W, N, M=None, seed=0, **over):
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.config import EnvConfig

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = N - 1 if M is None else M
            EnvConfig.__init__(self)
    return BatchedCollisionAvoidanceEnv(W, Cfg(), device="cuda:0", seed=seed, **over)


def _acts(rng, W, N, p_straight=0.8):
    a = rng.integers(0, 11, size=(W, N))
    a[rng.random((W, N)) < p_straight] = 2
    return a.astype(np.int32)


def _check_step(tag, out, ora, env, st, ep):
    obs, rew, done, go = [t.cpu().numpy() for t in out]
    oobs, orew, odone, ogo = ora
    assert np.array_equal(done, odone) and np.array_equal(go, ogo), tag
    assert rp.obs_diff(obs, oobs).max() <= OBS_TOL, tag
    assert np.array_equal(obs[..., :2], oobs[..., :2].astype(np.float32)), tag            # is_learning, num_other_agents exact
    assert np.abs(rew - orew).max() <= OBS_TOL, tag
    f64, f32, fl = [v.cpu().numpy() for v in env.get_state()]
    assert np.array_equal(fl.view(np.uint32), st.flags) and np.array_equal(f32, st.f32), tag
    np.testing.assert_allclose(f64, st.f64, rtol=0, atol=STATE_TOL, err_msg=str(tag))
    assert np.array_equal(env.episode.cpu().numpy().view(np.uint32), ep), tag


# the forms each case runs (last_step_form): (N, M, W, sort, pipe) -> (one step per launch, the K-step launch)
HORIZON_FORMS = {
    (4, None, 512, 0, None): ("QUAD", ("RELAY", 3)), (4, None, 512, 1, "1"): ("QUAD", ("PIPE", 0)),
    (4, None, 512, 0, "0"): ("QUAD", ("LOOP_PF", 0)), (4, None, 40000, 0, None): ("STEP", ("LOOP", 0)),
    (10, None, 300, 0, None): ("QUAD", ("PIPE", 0)), (10, 4, 300, 1, None): ("QUAD", ("PIPE", 0)),
    (6, None, 200, 2, None): ("QUAD", ("RELAY", 3)), (5, None, 256, 0, None): ("QUAD", ("LOOP", 0)),
}


@pytest.mark.parametrize("N,M,W,sort,pipe,over", [
    (4, None, 512, 0, None, dict()),                                              # relay kernel (BASELINE configs[1] shape)
    (4, None, 512, 1, "1", dict(gen_min_agents=2, gen_nonlearning_fraction=0.3)),  # two-wavefront pipeline, closest_first, scripted agents
    (4, None, 512, 0, "0", dict(gen_min_agents=2)),                               # single wavefront, register prefetch
    (4, None, 40000, 0, None, dict(gen_min_agents=2, gen_nonlearning_fraction=0.2)),   # beyond latency mode: the plain step loop
    (10, None, 300, 0, None, dict(gen_min_agents=2, gen_nonlearning_fraction=0.2)),    # configs[3] shape
    (10, 4, 300, 1, None, dict(gen_min_agents=5)),                                # horizon AND clipping to the 4 closest
    (6, None, 200, 2, None, dict(gen_min_agents=3)),                              # time-to-impact order
    (5, None, 256, 0, None, dict(gen_min_agents=2, gen_pool_size=0)),             # in-kernel generator
])
def test_finite_sensing_horizon_and_time_step_reward(N, M, W, sort, pipe, over, monkeypatch):
    if pipe is not None:
        monkeypatch.setenv("CAVOID_PIPELINE", pipe)
    seed, single, K = 29, 60, 40
    kw = dict(FIELDS, sort_method=sort, **over)
    env, twin = _env(W, N, M, seed=seed, **kw), _env(W, N, M, seed=seed, **kw)
    monkeypatch.delenv("CAVOID_PIPELINE", raising=False)
    ocfg, ogen = rp.oracle_for(N, M, **kw)
    st = co.State.empty(W, N)
    ep = np.zeros(W, np.uint32)
    co.generate(ocfg, ogen, seed, st, ep)
    o0 = env.reset().cpu().numpy()
    twin.reset()
    oo0 = co.observe(ocfg, st)
    assert rp.obs_diff(o0, oo0).max() <= OBS_TOL and np.array_equal(o0[..., 1], oo0[..., 1].astype(np.float32))
    rng = np.random.default_rng(seed)
    seen_fewer, stepped_pay = False, False
    # ---- one step per launch --------------------------------------------------------------------------------------------------
    for t in range(single):
        a = _acts(rng, W, N)
        out = env.step_autoreset(torch.from_numpy(a).cuda())
        assert env.last_step_form == (HORIZON_FORMS[(N, M, W, sort, pipe)][0], 0)
        ora = co.step_autoreset(ocfg, ogen, seed, st, ep, a)
        _check_step(("single", N, t), out, ora, env, st, ep)
        twin.step_autoreset(torch.from_numpy(a).cuda())
        present = (st.flags.reshape(W, N) & 0x20) != 0
        n_world = present.sum(axis=1, keepdims=True)
        seen_fewer |= bool((ora[0][..., 1][present] < np.minimum(np.broadcast_to(n_world - 1, present.shape)[present], ocfg.max_other)).any())
        stepped_pay |= bool(np.isclose(ora[1], -0.01).any())
    assert seen_fewer and stepped_pay          # the horizon really hid neighbours; the step reward really was paid
    # ---- K steps in ONE launch, every step in its slot (plain outputs) and as packed records -----------------------------------
    acts = np.stack([_acts(rng, W, N) for _ in range(K)])
    slots = env.new_step_slots(K)
    obs, rew, done, go = env.step_autoreset_n(torch.from_numpy(acts).cuda(), slots=slots)
    assert env.last_step_form == HORIZON_FORMS[(N, M, W, sort, pipe)][1]
    pslots = twin.new_step_slots(K, packed=True)
    twin.step_autoreset_packed(torch.from_numpy(acts).cuda(), pslots)
    assert twin.last_step_form == HORIZON_FORMS[(N, M, W, sort, pipe)][1]
    restarts = 0
    for t in range(K):
        oobs, orew, odone, ogo = co.step_autoreset(ocfg, ogen, seed, st, ep, acts[t])
        assert np.array_equal(done[t].cpu().numpy(), odone) and np.array_equal(go[t].cpu().numpy(), ogo), t
        assert rp.obs_diff(obs[t].cpu().numpy(), oobs).max() <= OBS_TOL, t
        assert np.array_equal(obs[t][..., 1].cpu().numpy(), oobs[..., 1].astype(np.float32)), t
        assert np.abs(rew[t].cpu().numpy() - orew).max() <= OBS_TOL, t
        restarts += int(ogo.sum())
    assert restarts > 0 or ep.max() >= 1
    assert np.array_equal(env.get_state()[2].cpu().numpy().view(np.uint32), st.flags)
    assert np.array_equal(env.episode.cpu().numpy().view(np.uint32), ep)
    width = env.obs_width
    assert torch.equal(pslots.packed[..., :width], obs) and torch.equal(pslots.packed[..., width], rew)
    assert torch.equal(pslots.packed[..., width + 1], done.float()) and torch.equal(pslots.game_over, go)
    env.close(); twin.close()


@pytest.mark.parametrize("N,M,W,over,steps", [
    (6, 2, 200, dict(FIELDS, gen_min_agents=4), (40, 40)),                          # M < N - 1 with a horizon (relay_coop_last's clip)
    (4, None, 300, dict(sort_method=1, gen_min_agents=3), (40, 40)),                # closest_first
    (5, None, 200, dict(dynamics=1, actions=WIDE, gen_min_agents=2), (40, 40)),     # unicycle_max_turn_rate: the relay's own clamp
    (4, None, 300, dict(evaluate_mode=1, gen_min_agents=2, gen_nonlearning_fraction=0.3), (40, 40)),
    (4, None, 256, dict(gen_min_agents=2), (129,)),                                 # one launch of 129 steps: the action ring wraps twice
])
def test_relay_kernel_configurations_against_the_oracle(N, M, W, over, steps):
    """env_relay_kernel (the default K-step form of these batches, asserted) straight against the float64 oracle in configurations
    the relay is not otherwise held to the oracle in; every step of every launch in its slot."""
    seed = 37
    env = _env(W, N, M, seed=seed, **over)
    ocfg, ogen = rp.oracle_for(N, M, **over)
    st = co.State.empty(W, N)
    ep = np.zeros(W, np.uint32)
    co.generate(ocfg, ogen, seed, st, ep)
    env.reset()
    rng = np.random.default_rng(seed)
    Mv = N - 1 if M is None else M
    clipped = hidden = False
    for K in steps:
        acts = np.stack([_acts(rng, W, N) for _ in range(K)])
        slots = env.new_step_slots(K)
        obs, rew, done, go = env.step_autoreset_n(torch.from_numpy(acts).cuda(), slots=slots)
        assert env.last_step_form == ("RELAY", 3)
        for t in range(K):
            oobs, orew, odone, ogo = co.step_autoreset(ocfg, ogen, seed, st, ep, acts[t])
            assert np.array_equal(done[t].cpu().numpy(), odone) and np.array_equal(go[t].cpu().numpy(), ogo), (K, t)
            assert rp.obs_diff(obs[t].cpu().numpy(), oobs).max() <= OBS_TOL, (K, t)
            assert np.array_equal(obs[t][..., 1].cpu().numpy(), oobs[..., 1].astype(np.float32)), (K, t)
            assert np.abs(rew[t].cpu().numpy() - orew).max() <= OBS_TOL, (K, t)
            n_world = ((st.flags.reshape(W, N) & 0x20) != 0).sum(axis=1)
            clipped |= bool((n_world - 1 > Mv).any())
            hidden |= bool((oobs[..., 1] < np.minimum(n_world - 1, Mv)[:, None]).any())
        f64, f32, fl = [v.cpu().numpy() for v in env.get_state()]
        assert np.array_equal(fl.view(np.uint32), st.flags) and np.array_equal(f32, st.f32), K
        np.testing.assert_allclose(f64, st.f64, rtol=0, atol=STATE_TOL)
        assert np.array_equal(env.episode.cpu().numpy().view(np.uint32), ep), K
    assert ep.max() >= 1                                    # worlds restarted inside the launches
    if M is not None:
        assert clipped and hidden                           # the clip and the horizon really hid neighbours
    env.close()


def test_time_step_reward_known_answer():
    """No oracle in the loop: a lone agent far from its goal is paid exactly reward_time_step per step; the step it arrives it is
    paid reward_at_goal instead (the published definition: the time penalty is the DEFAULT of a step, not an addend)."""
    env = _env(1, 1, reward_time_step=-0.01)
    f64 = torch.tensor([[0.0], [0.0], [0.0], [50.0]], dtype=torch.float64).cuda()
    f32 = torch.tensor([[0.55], [0.0], [0.3], [1.0], [0.0]], dtype=torch.float32).cuda()
    env.set_state(f64, f32, torch.tensor([0x20 | 0x40], dtype=torch.int32).cuda())
    a = torch.full((1, 1), 2, dtype=torch.int32).cuda()              # full speed straight ahead: 0.2 m per step
    _, r1, d1, _ = env.step(a)
    assert r1.item() == np.float32(-0.01) and d1.item() == 0         # 0.35 m to go
    _, r2, d2, _ = env.step(a)
    assert r2.item() == 1.0 and d2.item() == 1                       # 0.15 m <= NEAR_GOAL_THRESHOLD
    _, r3, _, _ = env.step(a)
    assert r3.item() == np.float32(-0.01)                            # at the goal already: the step's default again
    env.close()


def test_sensing_horizon_known_answer():
    """No oracle in the loop: three agents on a line, horizon 3 m.  The middle one sees both others, the outer ones only the
    middle one (centre distance 2.5 m; the far end is 5 m away)."""
    env = _env(1, 3, sensing_horizon=3.0)
    f64 = torch.tensor([[-2.5, 0.0, 2.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [50.0, 50.0, 50.0]], dtype=torch.float64).cuda()
    f32 = torch.tensor([[-2.5, 0.0, 2.5], [9.0, 9.0, 9.0], [0.3, 0.3, 0.3], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]], dtype=torch.float32).cuda()
    env.set_state(f64, f32, torch.full((3,), 0x20 | 0x40, dtype=torch.int32).cuda())
    row = env.observe()[0].cpu().numpy()
    assert row[:, 1].tolist() == [1.0, 2.0, 1.0]
    assert abs(row[0, 6 + 6] - 1.9) < 1e-6 and np.all(row[0, 6 + 7:] == 0)      # the one neighbour's gap; the second slot is empty
    far = _env(1, 3)
    far.set_state(f64, f32, torch.full((3,), 0x20 | 0x40, dtype=torch.int32).cuda())
    assert far.observe()[0, :, 1].cpu().tolist() == [2.0, 2.0, 2.0]
    env.close(); far.close()


# ---- every numeric field off its default (tests/cfg_regimes.py) ---------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.cid for c in R.select("tile-")])
def test_every_numeric_field_off_its_default_in_every_tile_form(cid, monkeypatch):
    """CLIPPED / UNCLIPPED with RING on the pool and the look-ahead rings and BOX generated inside the step: one step per launch, the
    K-step launch in slots and as packed records, every step against the oracle; the form of every launch against the case's table
    entry (cfg_regimes.TILE_SHAPES) -- a silent fallback fails."""
    case = R.BY_ID[cid]
    if case.pipe is not None:
        monkeypatch.setenv("CAVOID_PIPELINE", case.pipe)
    env = _env(case.W, case.N, seed=case.seed, **case.over)
    monkeypatch.delenv("CAVOID_PIPELINE", raising=False)
    run = R.drive_gpu(case, env, *case.forms)
    R.assert_events(case, run)
    env.close()


@pytest.mark.parametrize("pool", [0, 500, R.DEFAULT_POOL])
@pytest.mark.parametrize("gen_set", ["RING", "BOX"])
def test_reset_generator_parity_off_the_default_numbers(gen_set, pool):
    """tests/test_gpu_parity.py::test_reset_generator_parity with every numeric field of the generator off its default: flags and float32
    state exact, float64 state to 1e-12, the masked reset"""
    W, N, seed = 1000, 6, 99
    over = dict(R.GEN_SETS[gen_set], gen_pool_size=pool)
    ocfg, ogen = rp.oracle_for(N, None, **over)
    env = _env(W, N, seed=seed, **over)
    obs = env.reset().cpu().numpy()
    st = co.State.empty(W, N)
    co.generate(ocfg, ogen, seed, st, np.zeros(W, np.uint32))

    def same_state():
        f64, f32, fl = [v.cpu().numpy() for v in env.get_state()]
        assert np.array_equal(fl.view(np.uint32), st.flags) and np.array_equal(f32, st.f32)
        np.testing.assert_allclose(f64, st.f64, rtol=0, atol=1e-12)
    same_state()
    np.testing.assert_allclose(obs, co.observe(ocfg, st), rtol=0, atol=OBS_TOL)
    assert np.array_equal(env.episode.cpu().numpy(), np.zeros(W, np.int32))
    n_world = ((st.flags.reshape(W, N) & 0x20) != 0).sum(axis=1)
    assert set(n_world) == set(range(2, N + 1))                 # both box sizes (gen_box_large_from = 4) and every agent count
    mask = (np.arange(W) % 3 == 0).astype(np.uint8)             # a masked reset advances only the masked worlds
    obs2 = env.reset(torch.from_numpy(mask).cuda()).cpu().numpy()
    ep = mask.astype(np.uint32)
    co.generate(ocfg, ogen, seed, st, ep, mask)
    same_state()
    np.testing.assert_allclose(obs2, co.observe(ocfg, st), rtol=0, atol=OBS_TOL)
    assert np.array_equal(env.episode.cpu().numpy().view(np.uint32), ep)
    env.close()
