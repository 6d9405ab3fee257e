"""GPU tests of the fused evaluation loop (`cavoid_eval_run`, csrc/cavoid_eval.hpp; `ga3c.evaluate(fused=True)`): whole EVALUATE_MODE
rounds -- policy forward, argmax (or the Philox draw), env.step without auto-reset, outcome record, finished tiles leaving early -- in
launches of K env steps, against the same rounds driven step by step from the host (`evaluate(fused=False)`: `cavoid_policy_forward` +
`cavoid_step` + a look at the world buffer per step).  The kernel runs the very same statements per value, so everything is compared
BIT for bit: the result dict, every per-agent tensor, the world buffer the round leaves behind.

The networks are `NetworkVP_rnn` with their random initial weights and a bias on one policy logit, so that the argmax depends on the
observation but favours one behaviour: action 2 (full speed, straight ahead: goals and collisions), action 8 (turning on the spot:
timeouts), or none.  The step-by-step result of every (shape, network) is computed once and shared by the cases that need it."""
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

from tests import eval_twins as tw
from tests.eval_twins import MAX_STEPS, MIX, NETS, SPLS, _assert_same, _not_over, _outcomes, _StepLog
from tests.gpu_support import EINVAL, EUNSUPPORTED, OK, ROOT, _env as _crowd_env

pytestmark = pytest.mark.gpu

FAMILY = "eval_fused"            # this file's rounds in the one cache of step-by-step references


def _policy(cfg, net, seed=1234, policy_seed=77):
    return tw.policy(cfg, net, seed, policy_seed)


def _env(W, N, seed, **over):
    over.setdefault("evaluate_mode", 1)
    over.setdefault("max_time_ratio", 1.75)
    return _crowd_env(W, N, seed=seed, **over)


def _make(W, N, net, frozen, over):
    env = _env(W, N, 21, **over)
    return env, _policy(env.config, net), _policy(env.config, "free", seed=4321, policy_seed=0) if frozen else None


def _reference(W, N, net, greedy=True, frozen=False, **over):
    """evaluate(fused=False, details=True) of one (shape, network): result, final world buffer, the step log -- computed once"""
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate

    def compute():
        env, pol, fz = _make(W, N, net, frozen, over)
        log = _StepLog(env)
        res = evaluate(env, pol, rounds=1, greedy=greedy, max_steps=MAX_STEPS, frozen_policy=fz, details=True)
        out = (res, [t.clone() for t in env.get_state()], log)
        tw.close(env, pol, fz)
        return out
    return tw.cached(FAMILY, (W, N, net, greedy, frozen, tuple(sorted(over.items()))), compute)


def _fused(W, N, net, spl, greedy=True, frozen=False, **over):
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate
    env, pol, fz = _make(W, N, net, frozen, over)
    res = evaluate(env, pol, rounds=1, greedy=greedy, max_steps=MAX_STEPS, frozen_policy=fz, fused=True, steps_per_launch=spl, details=True)
    state = [t.clone() for t in env.get_state()]
    tw.close(env, pol, fz)
    return res, state


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
    pol = _policy(env.config, "free")
    why = evaluate_fused_unavailable_reason(env, pol, None)
    assert why is not None and "frozen" in why
    with pytest.raises(ValueError, match="frozen"):
        evaluate(env, pol, fused=True)
    env.reset()
    rec = _EvalRecords(env)
    rc = _raw(env, pol, rec, 4)
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
    return tw.raw("cavoid_eval_run", env, pol, rec, n, frozen, buffers=buffers, obs=obs)


def test_launch_edges_at_the_raw_entry_point():
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords
    W, N = 64, 4
    env = _env(W, N, 21)
    pol = _policy(env.config, "straight")
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
    wide = _policy(other.config, "free")
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


def test_train_cli_runs_the_kernel_and_prints_the_same_result():
    fused, plain = tw.cli(["--worlds", "64", "--fused-evaluate"]), tw.cli(["--worlds", "64"])
    assert "[Evaluate] fused evaluation kernel (cavoid_eval_run), 4 env steps per launch" in fused
    assert "cavoid_eval_run" not in plain
    last = tw.last_evaluate_line
    assert len(last(fused)) == 1 and last(fused) == last(plain)
    tw.report_cache(FAMILY)      # (a whole run of this file: 6 shapes x 3 networks, the two mixes x 3, two sampled rounds, the time-step reward: 27)
