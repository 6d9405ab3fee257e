"""Every env-step form against the C oracle AT its comparisons: the hand-placed worlds of tests/tie_regimes.py -- exact ties of the sort
keys (rank_exact behind __ballot(tie): T1..T8) and exact equality, one ulp below and one ulp above in every threshold predicate (P1..P9)
-- pushed with set_state into a batch of generator worlds.  tests/test_tie_regimes_host.py proves on the CPU that the cases are what they
claim to be.

Each subject pushes the batch three times and runs it: one step per launch, one K-step launch into per-step slots, the same launch as
packed records (K = tie_regimes.STEPS = 8: the relay's 8-slot ring once, its 4-slot ring twice; the thresholds are met at the 1st and the
4th step, T8's tie at the 3rd).  After observe() of the pushed state and after EVERY step: done, game_over, is_learning and the
neighbour count exact, WHO sits in every slot exact (the radius column, bit for bit: every placed agent has its own radius, so a swapped
order cannot hide inside the observation tolerance), observations (the ego heading on the circle) and rewards within 1e-5; after every
launch every flag bit, the float32 state and the episode counters exact, the float64 state within 1e-9, and the sign of a heading turned
to +-pi bit for bit.  Every launch asserts the form that ran: a silent fallback fails."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import replay as rp
from tests import tie_regimes as T

pytestmark = pytest.mark.gpu

OBS_TOL, STATE_TOL = 1e-5, 1e-9
ENV_VARS = ("CAVOID_QUAD", "CAVOID_PIPELINE", "CAVOID_RELAY_CONSUMERS", "CAVOID_PREFETCH_POOL", "CAVOID_WPW")
K = T.STEPS


def _make_env(monkeypatch, group, N, env_vars, **more):
    """tests/test_gpu_launch_forms.py::_make_env: the CAVOID_* switches are read by cavoid_create -- set for this env only"""
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.config import EnvConfig

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = T.M_of(group, N)
            EnvConfig.__init__(self)
    for k in ENV_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env_vars.items():
        monkeypatch.setenv(k, v)
    try:
        return BatchedCollisionAvoidanceEnv(T.num_worlds(group, N), Cfg(), device="cuda:0", seed=T.SEED, **dict(T.over_of(group), **more))
    finally:
        for k in ENV_VARS:
            monkeypatch.delenv(k, raising=False)


def _push(env, run):
    """the batch as the oracle run started from it, the episode counters back at 0"""
    env.seed(T.SEED, torch.zeros(env.num_worlds, dtype=torch.int32, device=env.device))
    st = run.start
    env.set_state(torch.from_numpy(st.f64).cuda(), torch.from_numpy(st.f32).cuda(), torch.from_numpy(st.flags.view(np.int32)).cuda())


def _rows(tag, obs, oobs):
    d = rp.obs_diff(obs, oobs)
    assert np.array_equal(obs[..., :2], oobs[..., :2].astype(np.float32)), (tag, "is_learning / num_other_agents")
    who, owho = obs[..., 10::7], oobs[..., 10::7].astype(np.float32)
    if not np.array_equal(who, owho):
        w, i = [int(v[0]) for v in np.nonzero((who != owho).any(axis=-1))]
        raise AssertionError((tag, "slot identity", "world %d agent %d" % (w, i), who[w, i].tolist(), owho[w, i].tolist()))
    if float(d.max()) > OBS_TOL:
        w, i, c = [int(v) for v in np.unravel_index(np.argmax(d), d.shape)]
        raise AssertionError((tag, "observation", "world %d agent %d column %d" % (w, i, c), float(obs[w, i, c]), float(oobs[w, i, c])))


def _step(tag, out, ora):
    obs, rew, done, go = out
    oobs, orew, odone, ogo = ora
    assert np.array_equal(done, odone) and np.array_equal(go, ogo), (tag, "done / game_over", np.nonzero(done != odone))
    bad = np.abs(rew - orew) > OBS_TOL
    assert not bad.any(), (tag, "reward", np.nonzero(bad), rew[bad].tolist(), orew[bad].tolist())
    _rows(tag, obs, oobs)


def _state(tag, env, run, t):
    f64, f32, fl = [v.cpu().numpy() for v in env.get_state()]
    st = run.states[t]
    bad = fl.view(np.uint32) != st.flags
    assert not bad.any(), (tag, "flags", np.nonzero(bad)[0].tolist(), fl[bad].tolist(), st.flags[bad].tolist())
    assert np.array_equal(f32, st.f32), (tag, "float32 state")
    assert float(np.abs(f64 - st.f64).max()) <= STATE_TOL, (tag, "float64 state", float(np.abs(f64 - st.f64).max()))
    assert np.array_equal(env.episode.cpu().numpy().view(np.uint32), run.eps[t]), (tag, "episode")
    for k, w in run.worlds():                                   # P8: the sign of a heading turned to +-pi, bit for bit
        if w.probe is not None and "hsign" in w.probe.read and t >= w.probe.step and run.eps[t][T.world_index(k)] == 0:
            a = T.world_index(k) * run.N + w.probe.host
            assert np.signbit(f64[2, a]) == np.signbit(st.f64[2, a]), (tag, w.name, f64[2, a], st.f64[2, a])
            if w.probe.role == "at":
                assert f64[2, a] == st.f64[2, a] and abs(f64[2, a]) == np.pi, (tag, w.name, f64[2, a], st.f64[2, a])


def hold(tag, env, run, single_form, k_form, packed_form=None, kinds=("single", "slots", "packed")):
    """the three runs of a subject; (form, consumers) of every launch asserted"""
    acts = torch.from_numpy(run.acts).cuda()
    wdt = env.obs_width
    env.reset()
    for kind in kinds:
        _push(env, run)
        _rows(tag + (kind, "observe"), env.observe().cpu().numpy(), run.obs0)
        if kind == "single":
            for t in range(K):
                out = env.step_autoreset(acts[t])
                assert env.last_step_form == single_form, (tag, kind, env.last_step_form)
                _step(tag + (kind, t), [v.cpu().numpy() for v in out], run.outs[t])
                _state(tag + (kind, t), env, run, t)
            continue
        slots = env.new_step_slots(K, packed=(kind == "packed"))
        if kind == "packed":
            pk, go = env.step_autoreset_packed(acts, slots)
            out = (pk[..., :wdt], pk[..., wdt], pk[..., wdt + 1].to(torch.uint8), go)
        else:
            out = env.step_autoreset_n(acts, slots=slots)
        want = k_form if kind == "slots" or packed_form is None else packed_form
        assert env.last_step_form == want, (tag, kind, env.last_step_form)
        out = [v.cpu().numpy() for v in out]
        for t in range(K):
            _step(tag + (kind, t), [v[t] for v in out], run.outs[t])
        _state(tag + (kind,), env, run, K - 1)


# ---- N = 4 x 512: every tile form ---------------------------------------------------------------------------------------------------
# form -> (CAVOID_* while the env is created, one step per launch, the K-step launch); tests/test_gpu_launch_forms.py::FORMS
QUAD0 = dict(CAVOID_QUAD="0")
TILE_FORMS = {
    "quad-relay3": (dict(), ("QUAD", 0), ("RELAY", 3)),           # the defaults of this shape (test_gpu_cfg_fields.py::HORIZON_FORMS)
    "step-relay2": (dict(QUAD0, CAVOID_PIPELINE="2", CAVOID_RELAY_CONSUMERS="2"), ("STEP", 0), ("RELAY", 2)),
    "step-relay4": (dict(QUAD0, CAVOID_PIPELINE="2", CAVOID_RELAY_CONSUMERS="4"), ("STEP", 0), ("RELAY", 4)),
    "step-pipe": (dict(QUAD0, CAVOID_PIPELINE="1"), ("STEP", 0), ("PIPE", 0)),
    "step-loop-pf": (dict(QUAD0, CAVOID_PIPELINE="0"), ("STEP", 0), ("LOOP_PF", 0)),
    "step-loop": (dict(QUAD0, CAVOID_PREFETCH_POOL="0"), ("STEP", 0), ("LOOP", 0)),
}
U4_GROUPS = ("u4", "u4-cd25")                                     # the relay does not carry U4 flipped: it hands the launch to PIPE


@pytest.mark.parametrize("name", list(T.GROUPS))
@pytest.mark.parametrize("form", list(TILE_FORMS))
def test_ties_and_thresholds_in_every_tile_form(form, name, monkeypatch):
    env_vars, single_form, k_form = TILE_FORMS[form]
    if name in U4_GROUPS and k_form[0] == "RELAY":
        k_form = ("PIPE", 0)
    group = T.GROUPS[name]
    run = T.Run.of(name, 4)
    env = _make_env(monkeypatch, group, 4, env_vars)
    hold((form, name), env, run, single_form, k_form)
    env.close()


# ---- other agent counts: the placed agents first, the rest absent, and the line of N -----------------------------------------------
# N -> (one step per launch, the K-step launch in slots, as packed records) with the default switches
#   5: the largest one-step form with mirrored distances; 6: key parking begins, 4-slot relay ring; 10: PIPE; 16: the largest tile (its
#   one-step launch is the plain step, not the quad step)
N_FORMS = {5: (("QUAD", 0), ("RELAY", 3), ("RELAY", 3)), 6: (("QUAD", 0), ("RELAY", 3), ("RELAY", 3)),
           10: (("QUAD", 0), ("PIPE", 0), ("PIPE", 0)), 16: (("STEP", 0), ("PIPE", 0), ("PIPE", 0))}
N_GROUPS = ("main", "horizon", "near-m2", "tti", "exact-gap", "u4")


@pytest.mark.parametrize("name", N_GROUPS)
@pytest.mark.parametrize("N", list(N_FORMS))
def test_ties_and_thresholds_at_other_agent_counts(N, name, monkeypatch):
    single_form, k_form, packed_form = N_FORMS[N]
    if name in U4_GROUPS and k_form[0] == "RELAY":
        k_form = packed_form = ("PIPE", 0)
    run = T.Run.of(name, N)
    env = _make_env(monkeypatch, T.GROUPS[name], N, {})
    hold((N, name), env, run, single_form, k_form, packed_form)
    env.close()


# ---- the crowd form -----------------------------------------------------------------------------------------------------------------
CROWD_GROUPS = ("main", "near", "tti")                            # sort methods 0, 1, 2


@pytest.mark.parametrize("name,rvo", [(g, 0) for g in CROWD_GROUPS] + [("main", 2)])
@pytest.mark.parametrize("N", [17, 33, 64])                       # three, one and one world per wavefront
def test_ties_and_thresholds_in_the_crowd_form(N, name, rvo, monkeypatch):
    """rvo = 2: the wave-cooperative ORCA programme compiled in (CROWD_RVO), the placed agents still static or learners"""
    form = ("CROWD_RVO" if rvo else "CROWD", 0)
    run = T.Run.of(name, N)
    env = _make_env(monkeypatch, T.GROUPS[name], N, {}, **(dict(rvo_enabled=rvo) if rvo else {}))
    hold((N, name, rvo), env, run, form, form)
    env.close()


# ---- the fused env step + experience push (cavoid_step_push; crowd_push_kernel above 16 agents) ----------------------------------
@pytest.mark.parametrize("N,name", [(4, "main"), (4, "tti"), (4, "near-m2"), (17, "main"), (17, "near")])
def test_ties_and_thresholds_in_the_fused_step_and_push(N, name, monkeypatch):
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    run = T.Run.of(name, N)
    env = _make_env(monkeypatch, T.GROUPS[name], N, {})
    roll = BatchedRollout(env, None, reflush_done=False)
    assert roll.step_path == "step_push", roll.step_path
    roll.reset()
    _push(env, run)
    acts = torch.from_numpy(run.acts).cuda()
    values = torch.zeros((env.num_worlds, N), dtype=torch.float32, device=env.device)
    for t in range(K):
        rew, done, go = roll.step(acts[t], values)
        _step((N, name, "step_push", t), [v.cpu().numpy() for v in (roll.obs, rew, done, go)], run.outs[t])
        _state((N, name, "step_push", t), env, run, t)
    if N > 16:
        assert env.last_step_form == ("CROWD", 0), env.last_step_form
    roll.close(); env.close()


# ---- the closed actor loops: run_fused (N = 4) and run_fused_crowd (N = 17) -------------------------------------------------------
def _actor(monkeypatch, group, N):
    """a greedy rollout on a network whose output layer has zero weights and a bias of +30 on the straight-ahead action: every learner
    goes straight whatever it observes"""
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    env = _make_env(monkeypatch, group, N, {})
    torch.manual_seed(1234)
    net = NetworkVP_rnn(env.config).to("cuda:0")
    with torch.no_grad():
        net.p_kernel.zero_()
        net.p_bias.zero_()
        net.p_bias[T.STRAIGHT] = 30.0
    roll = BatchedRollout(env, FusedPolicy(net, seed=77), reflush_done=False, greedy=True, skip_finished=True)
    roll.reset()
    return env, roll


@pytest.mark.parametrize("N,name", [(4, "main"), (4, "tti"), (4, "near-m2"), (17, "main"), (17, "near")])
def test_ties_and_thresholds_in_the_closed_actor_loops(N, name, monkeypatch):
    """K closed-loop steps in ONE launch against the step-by-step twin, bit for bit (tests/test_gpu_actor.py's comparison), and the twin's
    every step -- observations, rewards, done, game_over, every flag bit -- against the oracle run in which every agent goes straight"""
    group = T.GROUPS[name]
    run = T.Run.of(name, N, straight=True)
    env_a, a = _actor(monkeypatch, group, N)
    env_b, b = _actor(monkeypatch, group, N)
    crowd = N > 16
    if crowd:
        assert a.crowd_fused_available, a.crowd_fused_unavailable_reason
    else:
        assert a.fused_available and a.actor_path.startswith("fused actor kernel"), a.actor_path
    for e in (env_a, env_b):
        _push(e, run)
        _rows((N, name, "observe"), e.observe().cpu().numpy(), run.obs0)         # (env.obs is the buffer the rollout acts on first)
    (a.run_fused_crowd if crowd else a.run_fused)(K)
    for t in range(K):
        rew, done, go = b.step()
        _step((N, name, "twin", t), [v.cpu().numpy() for v in (b.obs, rew, done, go)], run.outs[t])
        _state((N, name, "twin", t), env_b, run, t)
    assert torch.equal(a.obs, b.obs), "obs"
    for x, y in zip(env_a.get_state(), env_b.get_state()):
        assert torch.equal(x, y), "state"
    for what in ("episode", "rewards", "done", "game_over"):
        assert torch.equal(getattr(env_a, what), getattr(env_b, what)), what
    for what in ("x", "val", "ret", "act_ring", "emit_t"):
        assert torch.equal(getattr(a, what), getattr(b, what)), what
    _state((N, name, "fused"), env_a, run, K - 1)
    if crowd:
        assert env_a.last_step_form == ("CROWD", 0) and env_b.last_step_form == ("CROWD", 0)
    a.close(); b.close(); env_a.close(); env_b.close()
