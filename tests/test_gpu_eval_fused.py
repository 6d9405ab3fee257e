"""GPU tests of the fused evaluation loop (`cavoid_eval_run`, csrc/cavoid_eval.hpp; `ga3c.evaluate(fused=True)`): whole EVALUATE_MODE
rounds -- policy forward, argmax (or the Philox draw), env.step without auto-reset, outcome record, finished tiles leaving early -- in
launches of K env steps, against the same rounds driven step by step from the host (`evaluate(fused=False)`: `cavoid_policy_forward` +
`cavoid_step` + a look at the world buffer per step).  The kernel runs the very same statements per value, so everything is compared
BIT for bit: the result dict, every per-agent tensor, the world buffer the round leaves behind.

The networks are `NetworkVP_rnn` with their random initial weights and a bias on one policy logit, so that the argmax depends on the
observation but favours one behaviour: action 2 (full speed, straight ahead: goals and collisions), action 8 (turning on the spot:
timeouts), or none.  The step-by-step result of every (shape, network) is computed once and shared by the cases that need it."""
import ctypes as C
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -4
MAX_STEPS = 400
BIAS = 1.0                       # on the favoured logit (the initial weights' logits spread over a few tenths)
NETS = {"straight": 2, "turn": 8, "free": None}
SPLS = (1, 7, 16)                # 7 divides no episode length in particular: launches begin on part-finished tiles


def _cfg_class(N):
    from rl_collision_avoidance_amd.config import EnvConfig

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            EnvConfig.__init__(self)
    return Cfg()


def _policy(cfg, bias_action, seed=1234, policy_seed=77):
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    net = NetworkVP_rnn(cfg, seed=seed).to("cuda:0")
    if bias_action is not None:
        with torch.no_grad():
            net.p_bias[bias_action] += BIAS
    return FusedPolicy(net, seed=policy_seed)


def _env(W, N, seed, **over):
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    over.setdefault("evaluate_mode", 1)
    over.setdefault("max_time_ratio", 1.75)
    return BatchedCollisionAvoidanceEnv(W, _cfg_class(N), device="cuda:0", seed=seed, **over)


class _StepLog(object):
    """wraps env.step of the step-by-step twin: every step's rewards and game_over flags, as the loop saw them"""

    def __init__(self, env):
        self.rew, self.over, self._step = [], [], env.step
        env.step = self

    def __call__(self, actions):
        out = self._step(actions)
        self.rew.append(out[1].clone().view(-1)); self.over.append(out[3].clone())
        return out

    def masked_return(self, N):
        """(the return as include/cavoid.h defines it, restated on the host: the float64 sum, in step order, of the rewards of the steps
        before which the agent's world was not over; which agents the loop paid something AFTER their world was over)"""
        want = torch.zeros_like(self.rew[0], dtype=torch.float64)
        paid_after = torch.zeros_like(self.rew[0], dtype=torch.bool)
        running = torch.ones_like(self.over[0], dtype=torch.bool)
        for rew, over_t in zip(self.rew, self.over):
            live = running.repeat_interleave(N)
            want += torch.where(live, rew.double(), torch.zeros_like(want))
            paid_after |= ~live & (rew != 0)
            running &= over_t == 0
        return want, paid_after

    def world_steps(self):
        """the step at which each world was over (the step count of the round where it never was)"""
        over = torch.stack(self.over).bool()                                   # [T, W]
        first = torch.where(over.any(0), over.int().argmax(0) + 1, torch.full_like(over[0], len(self.over), dtype=torch.int64))
        return first.to(torch.int32)


_REFS = {}


def _reference(W, N, net, greedy=True, frozen=False, **over):
    """evaluate(fused=False, details=True) of one (shape, network): result, final world buffer, the step log -- computed once"""
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate
    key = (W, N, net, greedy, frozen, tuple(sorted(over.items())))
    if key not in _REFS:
        env = _env(W, N, 21, **over)
        pol = _policy(env.config, NETS[net])
        fz = _policy(env.config, None, seed=4321, policy_seed=0) if frozen else None
        log = _StepLog(env)
        res = evaluate(env, pol, rounds=1, greedy=greedy, max_steps=MAX_STEPS, frozen_policy=fz, details=True)
        _REFS[key] = (res, [t.clone() for t in env.get_state()], log)
        pol.close()
        if fz is not None:
            fz.close()
        env.close()
    return _REFS[key]


def _fused(W, N, net, spl, greedy=True, frozen=False, **over):
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate
    env = _env(W, N, 21, **over)
    pol = _policy(env.config, NETS[net])
    fz = _policy(env.config, None, seed=4321, policy_seed=0) if frozen else None
    res = evaluate(env, pol, rounds=1, greedy=greedy, max_steps=MAX_STEPS, frozen_policy=fz, fused=True, steps_per_launch=spl, details=True)
    state = [t.clone() for t in env.get_state()]
    pol.close()
    if fz is not None:
        fz.close()
    env.close()
    return res, state


def _assert_same(ref, ref_state, got, got_state, what, log=None, skip=()):
    """Everything bit for bit.  The return (``per_agent["ret"]``, ``mean_reward``) is held to the step-by-step run twice: bitwise to the
    loop's own sum for every agent the loop paid nothing after its world was over -- and, with ``log``, bitwise to the definition of
    include/cavoid.h (the rewards up to and including the step at which the world is over) for EVERY agent.  The two differ where
    cavoid_step goes on paying a finished world: at the default rewards that is the getting-close penalty of an agent that ran out of
    time within 0.2 m of another (measured: 10 x 48 box scenarios, unbiased network: loop mean_reward -0.19782, kernel -0.13149; the
    4 x 64 scripted mixes likewise), with reward_time_step every agent (test_return_stops_where_the_world_is_over)."""
    masked, paid_after = (None, None)
    if log is not None:
        masked, paid_after = log.masked_return(ref_state[2].numel() // log.over[0].numel())
        if bool(paid_after.any()):
            print("%s: the loop paid %d agent(s) after their world was over; mean_reward loop %.17g kernel %.17g"
                  % (what, int(paid_after.sum()), ref["mean_reward"], got["mean_reward"]))
            skip = tuple(skip) + ("mean_reward", "ret")
    for k in ref:
        if k == "per_agent" or k in skip:
            continue
        assert type(ref[k]) is type(got[k]) and ref[k] == got[k], (what, k, ref[k], got[k])
    assert list(ref) == list(got)
    for k, t in ref["per_agent"].items():
        if k in skip:
            continue
        assert t.dtype == got["per_agent"][k].dtype and torch.equal(t, got["per_agent"][k]), (what, "per_agent", k)
    if masked is not None:
        learning = ref["per_agent"]["learning"]
        assert torch.equal(got["per_agent"]["ret"], masked), (what, "ret against its definition")
        assert got["mean_reward"] == float(masked[learning].sum()) / max(int(learning.sum()), 1), (what, "mean_reward")
        assert torch.equal(got["per_agent"]["ret"][~paid_after], ref["per_agent"]["ret"][~paid_after]), (what, "ret against the loop's")
    for name, a, b in zip(("f64", "f32", "flags"), ref_state, got_state):
        assert torch.equal(a, b), (what, "final state", name)


def _outcomes(res):
    per = res["per_agent"]
    return set(per["outcome"][per["learning"]].tolist())


def _check_not_empty(W, N, over, frozen=False):
    """the step-by-step results a pass must not be empty of: early exit happened, and the three networks together saw every outcome"""
    from rl_collision_avoidance_amd.ga3c.evaluate import OUTCOME_COLLISION, OUTCOME_GOAL, OUTCOME_TIMEOUT
    seen = set()
    spread = False
    for net in NETS:
        res, _, log = _reference(W, N, net, frozen=frozen, **over)
        seen |= _outcomes(res)
        ws = log.world_steps()
        assert int(ws.max()) == res["env_steps"] <= MAX_STEPS
        print("%dx%d %-8s env_steps %d world_steps min %d median %d distinct %d outcomes %s" % (
            N, W, net, res["env_steps"], int(ws.min()), int(ws.median()), ws.unique().numel(), sorted(_outcomes(res))))
        if ws.unique().numel() >= 3 and 2 * int(ws.min()) < int(ws.max()):
            spread = True
        if net == "straight":      # the network that ends worlds early: its round must show the spread early exit is about
            assert ws.unique().numel() >= 3 and 2 * int(ws.min()) < int(ws.max()), (ws.unique().tolist())
    assert spread
    assert {OUTCOME_GOAL, OUTCOME_COLLISION, OUTCOME_TIMEOUT} <= seen, seen


SHAPES = {
    "n2": (96, 2, dict()),
    "n4_quad": (64, 4, dict()),
    "n5_2to5_present": (60, 5, dict(gen_min_agents=2)),
    "n10_box": (48, 10, dict(gen_mode=1)),
    "n16": (32, 16, dict()),
    "n4_ragged": (13, 4, dict()),                       # one ragged tile (13 of 16 worlds); with 13 worlds spread thinner, tiles past the end
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_round_equals_step_by_step(shape):
    W, N, over = SHAPES[shape]
    _check_not_empty(W, N, over)
    for net in NETS:
        ref, ref_state, log = _reference(W, N, net, **over)
        for spl in SPLS:
            got, got_state = _fused(W, N, net, spl, **over)
            _assert_same(ref, ref_state, got, got_state, (shape, net, spl), log)


def test_fused_round_acts_on_more_than_one_action(monkeypatch):
    """N = 4, one step per launch: the actions buffer after every launch -- the argmax really depends on the observation"""
    from rl_collision_avoidance_amd.ga3c import evaluate as ev
    W, N, over = SHAPES["n4_quad"]
    most = {"n": 0, "launches": 0}
    run = ev.eval_run

    def spy(env, policy, frozen_policy, rec, n_steps, greedy=True):
        run(env, policy, frozen_policy, rec, n_steps, greedy)
        assert n_steps == 1
        most["n"] = max(most["n"], int(rec.actions.unique().numel()))
        most["launches"] += 1
    monkeypatch.setattr(ev, "eval_run", spy)
    ref, ref_state, log = _reference(W, N, "free", **over)
    got, got_state = _fused(W, N, "free", 1, **over)
    _assert_same(ref, ref_state, got, got_state, "free, one step per launch", log)
    assert most["launches"] == ref["env_steps"]              # one launch per step, none after the last world was over
    assert most["n"] >= 3, most


_CHILD = """
import sys
sys.path.insert(0, %r)
from tests import test_gpu_eval_fused as t
W, N, over = t.SHAPES["n4_quad"]
for net in t.NETS:
    ref, ref_state, log = t._reference(W, N, net, **over)
    for spl in t.SPLS:
        got, got_state = t._fused(W, N, net, spl, **over)
        t._assert_same(ref, ref_state, got, got_state, (net, spl), log)
print("SAME")
"""


def test_fused_round_equals_step_by_step_on_one_wavefront(tmp_path):
    """4 x 64 with CAVOID_ACTOR_QUAD=0 (read at the launch): the tile's env step by wavefront 0 alone, in a child process"""
    script = tmp_path / "quad0.py"
    script.write_text(_CHILD % ROOT)
    run = subprocess.run([sys.executable, str(script)], cwd=ROOT, env=dict(os.environ, CAVOID_ACTOR_QUAD="0"), timeout=300,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-3000:])
    assert run.returncode == 0 and run.stdout.strip().endswith("SAME")


MIX = dict(gen_min_agents=2, gen_nonlearning_fraction=0.5, rvo_enabled=1, gen_rvo_fraction=0.34, gen_static_fraction=0.33)


@pytest.mark.parametrize("frozen", [False, True])
def test_scripted_and_frozen_agents(frozen):
    """4 x 64 among static / non-cooperative / ORCA agents (the ORCA instantiation); with frozen-network agents and their network
    (the frozen instantiation)"""
    over = dict(MIX, gen_frozen_fraction=0.3) if frozen else dict(MIX)
    for net in NETS:
        ref, ref_state, log = _reference(64, 4, net, frozen=frozen, **over)
        assert log.world_steps().unique().numel() >= 3
        for spl in SPLS:
            got, got_state = _fused(64, 4, net, spl, frozen=frozen, **over)
            _assert_same(ref, ref_state, got, got_state, (frozen, net, spl), log)
    if frozen:               # the scripted agents really were of every kind, frozen-network ones among them
        from rl_collision_avoidance_amd import _lib
        pol = (ref_state[2] >> _lib.F_POLICY_SHIFT) & _lib.F_POLICY_MASK
        present = (ref_state[2] & _lib.F_PRESENT) != 0
        assert set(pol[present].tolist()) >= {_lib.POLICY_EXTERNAL, _lib.POLICY_FROZEN_NET}


def test_frozen_agents_without_their_network_are_refused():
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords, evaluate, evaluate_fused_unavailable_reason
    from rl_collision_avoidance_amd import _lib
    env = _env(64, 4, 21, **dict(MIX, gen_frozen_fraction=0.3))
    pol = _policy(env.config, None)
    why = evaluate_fused_unavailable_reason(env, pol, None)
    assert why is not None and "frozen" in why
    with pytest.raises(ValueError, match="frozen"):
        evaluate(env, pol, fused=True)
    env.reset()
    rec = _EvalRecords(env)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = _lib.lib().cavoid_eval_run(env._h, pol._h, None, C.byref(rec.c), p(env.obs), p(env.rewards), p(env.done), p(env.game_over),
                                    p(rec.actions), p(rec.values), 4, 1, env._stream())
    assert rc == EUNSUPPORTED
    pol.close(); env.close()


def test_sampled_evaluation():
    """greedy=False: the Philox draw of (seed, row, step counter + t) -- the same numbers as the step-by-step path draws"""
    for net in ("straight", "free"):
        ref, ref_state, log = _reference(64, 4, net, greedy=False)
        got, got_state = _fused(64, 4, net, 7, greedy=False)
        _assert_same(ref, ref_state, got, got_state, ("sampled", net), log)
    # (and the draw matters: the sampled round is not the greedy one)
    greedy = _reference(64, 4, "free")[0]
    assert not torch.equal(greedy["per_agent"]["ret"], ref["per_agent"]["ret"]) or greedy["env_steps"] != ref["env_steps"]


def test_return_stops_where_the_world_is_over():
    """reward_time_step = -0.01: cavoid_step pays every present agent every step, finished worlds too.  The kernel's return is the
    float64 sum, in step order, of the rewards of the steps before which the agent's world was not over; the loop's sums on."""
    over = dict(reward_time_step=-0.01)
    ref, ref_state, log = _reference(64, 4, "straight", **over)
    got, got_state = _fused(64, 4, "straight", 7, **over)
    _assert_same(ref, ref_state, got, got_state, "time-step reward", skip=("mean_reward", "ret"))
    want, paid_after = log.masked_return(4)
    assert int(paid_after.sum()) > 64                        # (every present agent of every world that ended early)
    assert torch.equal(got["per_agent"]["ret"], want)
    assert not torch.equal(got["per_agent"]["ret"], ref["per_agent"]["ret"])          # (why include/cavoid.h spells the definition out)
    learning = ref["per_agent"]["learning"]
    assert got["mean_reward"] == float(want[learning].sum()) / max(int(learning.sum()), 1)
    assert got["mean_reward"] > ref["mean_reward"]                                    # the loop went on charging finished worlds


def _raw(env, pol, rec, n, frozen=None, buffers=None, obs=None):
    from rl_collision_avoidance_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    return _lib.lib().cavoid_eval_run(env._h, pol._h if pol is not None else None, frozen._h if frozen is not None else None,
                                      C.byref(buffers if buffers is not None else rec.c), p(env.obs if obs is None else obs), p(env.rewards),
                                      p(env.done), p(env.game_over), p(rec.actions), p(rec.values), n, 1, env._stream())


def _not_over(env):
    """worlds not over, from the world buffer: cavoid_step's game_over predicate in EVALUATE_MODE"""
    from rl_collision_avoidance_amd import _lib
    fl = env.get_state()[2].view(env.num_worlds, env.max_agents)
    running = ((fl & _lib.F_PRESENT) != 0) & ((fl & _lib.F_DONE_MASK) == 0)
    return running.any(1)


def test_launch_edges_at_the_raw_entry_point():
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords
    W, N = 64, 4
    env = _env(W, N, 21)
    pol = _policy(env.config, NETS["straight"])
    env.reset()
    rec = _EvalRecords(env)
    snap = lambda: [t.clone() for t in (*env.get_state(), env.obs, rec.ret, rec.goal_step, rec.world_steps, rec.worlds_running, rec.actions)]
    # n_steps == 0: OK, nothing touched (not even the running count)
    rec.worlds_running.fill_(-7)
    before = snap()
    assert _raw(env, pol, rec, 0) == OK
    assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    # argument errors
    bad = _lib.CavoidEvalBuffers.from_buffer_copy(rec.c)
    bad.struct_size += 8
    assert _raw(env, pol, rec, 4, buffers=bad) == EINVAL
    for field in ("ret", "goal_step", "world_steps", "worlds_running"):
        bad = _lib.CavoidEvalBuffers.from_buffer_copy(rec.c)
        setattr(bad, field, None)
        assert _raw(env, pol, rec, 4, buffers=bad) == EINVAL, field
    assert _raw(env, None, rec, 4) == EINVAL
    other = _env(16, 5, 3)                                   # handles that do not describe the same batch: a policy of another width
    wide = _policy(other.config, None)
    assert _raw(env, wide, rec, 4) == EINVAL
    assert _raw(env, pol, rec, -1) == EINVAL
    assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    wide.close(); other.close()
    # chunks of 7: after each, the running count is the world buffer's, and world_steps moved only in the worlds that were running
    rec.worlds_running.zero_()
    done_steps, counts = 0, []
    while done_steps < MAX_STEPS:
        was = _not_over(env)
        ws0 = rec.world_steps.clone()
        assert _raw(env, pol, rec, 7) == OK
        done_steps += 7
        now = _not_over(env)
        counts.append(int(rec.worlds_running.item()))
        assert counts[-1] == int(now.sum())
        moved = rec.world_steps - ws0
        assert bool((moved[~was] == 0).all()) and bool((moved[was] >= 1).all()) and bool((moved[now] == 7).all()) and int(moved.max()) <= 7
        if counts[-1] == 0:
            break
    assert counts[-1] == 0 and len(counts) >= 3 and any(0 < c < W for c in counts)   # launches began on part-finished batches
    assert sorted(counts, reverse=True) == counts
    # a launch on worlds that are all over: state, records and obs unchanged, nobody running
    before = snap()
    assert _raw(env, pol, rec, 16) == OK
    after = snap()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert int(rec.worlds_running.item()) == 0
    # the records are the step-by-step round's
    ref, _, log = _reference(W, N, "straight")
    assert torch.equal(rec.world_steps, log.world_steps().to(rec.world_steps.device))
    assert torch.equal(rec.ret, log.masked_return(N)[0])
    pol.close(); env.close()


def _cli(extra):
    cmd = [sys.executable, "-m", "rl_collision_avoidance_amd.ga3c.train", "--worlds", "64", "--evaluate", "1"] + extra
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    run = subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-3000:])
    assert run.returncode == 0
    return run.stdout


def test_train_cli_runs_the_kernel_and_prints_the_same_result():
    fused, plain = _cli(["--fused-evaluate"]), _cli([])
    assert "[Evaluate] fused evaluation kernel (cavoid_eval_run), 4 env steps per launch" in fused
    assert "cavoid_eval_run" not in plain
    last = lambda out: [l for l in out.splitlines() if l.startswith("[Evaluate] agents ")]
    assert len(last(fused)) == 1 and last(fused) == last(plain)
