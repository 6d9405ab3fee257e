"""GPU tests of the fused evaluation loop of crowd worlds (`cavoid_crowd_eval_run`, csrc/cavoid_crowd_eval.hpp;
`ga3c.evaluate(fused_crowd=True)`): whole EVALUATE_MODE rounds of worlds of 17..64 agents -- the ring form of the policy pass, argmax (or
the Philox draw), the crowd env.step without auto-reset, the outcome record, finished tiles leaving early -- in launches of K env steps,
against the same rounds driven step by step from the host (`evaluate()`: `cavoid_policy_forward` + `cavoid_step` + a look at the world
buffer per step: code this kernel does not touch).  The kernel runs the very same statements per value, so everything is compared BIT for
bit: the result dict, every per-agent tensor, the world buffer the round leaves behind, and the observation the kernel left of the worlds
that ended at the round's last step.  The pattern, the step log and the comparison are tests/test_gpu_eval_fused.py's.

The networks are `NetworkVP_rnn` with their random initial weights and that file's bias on one policy logit ("straight": full speed ahead,
"turn": turning on the spot, "free": none).  The step-by-step result of every case is computed once and shared."""
import ctypes as C
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

from tests import eval_twins as tw
from tests.eval_twins import MAX_STEPS, _not_over, _outcomes
from tests.gpu_support import EINVAL, EUNSUPPORTED, OK, ROOT, _env as _crowd_env

pytestmark = pytest.mark.gpu

ORCA = dict(rvo_enabled=2, gen_rvo_fraction=0.5, gen_nonlearning_fraction=0.5)

# name: (N, W, M, env settings, network, max_time_ratio, steps per launch).  The shapes are the smallest at which the lane mapping, the
# ring or the recorder can go wrong.  Network and max_time_ratio are chosen per case so that the STEP-BY-STEP round has what the case is
# compared on (test_the_step_by_step_rounds_are_not_empty); the reason stands beside each.
CASES = {
    # three worlds per tile, 13 idle lanes, a ragged last tile, absent slots, scripted agents.  "straight" at the default ratio: sparse worlds
    # (2..17 agents) are where agents of an untrained network reach goals; worlds end between step 16 and the cut at 400
    "n17_three_worlds": (17, 50, 16, dict(gen_min_agents=2, gen_nonlearning_fraction=0.3), "straight", 1.75, (1, 7, 16)),
    # two worlds per tile, box scenarios.  "free", ratio 0.5: a short round (73 steps) of collisions and time-outs, and the loop pays
    # agents that ran out of time beside another after their world's end (the two definitions of the return differ)
    "n22_box": (22, 33, 21, dict(gen_mode=1, gen_pool_size=0), "free", 0.5, (7,)),
    # the ring's first refill.  "turn", ratio 0.4: nobody leaves its place, every agent runs out of time -- a world ends by its slowest clock
    "n25_first_refill": (25, 21, 24, dict(), "turn", 0.4, (16,)),
    # one world per tile, 31 idle lanes.  "straight", ratio 0.5: collisions and time-outs; the slowest worlds are cut at 400 (unfinished agents)
    "n33_one_world": (33, 20, 32, dict(), "straight", 0.5, (7,)),
    # M < N - 1: the observation clips to the 19 nearest (an ordinary policy handle).  "free", ratio 0.4: every world ends before the cut
    "n33_m19": (33, 20, 19, dict(), "free", 0.4, (16,)),
    # a slot refilled twice.  "straight", ratio 0.4: collisions and time-outs, worlds end from step 260 on
    "n48_two_refills": (48, 10, 47, dict(), "straight", 0.4, (7,)),
    # all 64 lanes, the full-width world mask, absent slots.  "straight" at the default ratio: goals in the sparse worlds, every outcome
    "n64_full_mask": (64, 12, 63, dict(gen_min_agents=2), "straight", 1.75, (16,)),
    # ORCA agents, both buckets (the <32, true> and <64, true> instantiations).  "free" / "straight", ratio 0.5: half the agents are scripted
    # and go on being paid by the loop after their world's end
    "n20_orca": (20, 30, 19, dict(ORCA), "free", 0.5, (7,)),
    "n40_orca": (40, 12, 39, dict(ORCA), "straight", 0.5, (16,)),
    # 520 workgroups: two per CU on every CU.  "turn", ratio 0.2: the shortest round (181 steps) that still ends worlds at 102 different steps
    "n33_two_per_cu": (33, 520, 32, dict(), "turn", 0.2, (16,)),
}
SAMPLED = ("n22_box", 7)             # the sampled case: greedy=False on this shape


_policy = tw.policy


def _make(name, **more):
    N, W, M, over, net, ratio, _ = CASES[name]
    env = _crowd_env(W, N, M, seed=21, evaluate_mode=1, max_time_ratio=ratio, **dict(over, **more))
    return env, _policy(env.config, net)


# the step-by-step round of every case is computed once (family "crowd_eval" of the one cache); no frozen policy in this form
ROUNDS = tw.CrowdRounds("crowd_eval", CASES, lambda name: _make(name) + (None,), switch="fused_crowd",
                        reason="evaluate_fused_crowd_unavailable_reason", run="eval_run_crowd")
_reference, _same_round = ROUNDS.reference, ROUNDS.same_round


def test_the_step_by_step_rounds_are_not_empty():
    """Conditions on the STEP-BY-STEP side (code of before), so that no comparison below passes on nothing: the cases together see every
    outcome, every case ends its worlds at different steps (early exit happened), and in at least one the loop paid an agent after its
    world was over (the two definitions of the return differ)."""
    from rl_collision_avoidance_amd.ga3c.evaluate import OUTCOME_COLLISION, OUTCOME_GOAL, OUTCOME_TIMEOUT
    seen, paid = set(), 0
    for name, (N, W, M, over, net, ratio, _) in CASES.items():
        res, state, log, _, _ = _reference(name)
        ws = log.world_steps()
        masked, paid_after = log.masked_return(N)
        out = _outcomes(res)
        print("%-18s N %2d W %3d M %2d %-8s ratio %.2f: env_steps %3d world_steps min %3d median %3d distinct %2d outcomes %s learning %d paid after %d" % (
            name, N, W, M, net, ratio, res["env_steps"], int(ws.min()), int(ws.median()), ws.unique().numel(), sorted(out),
            res["agents"], int(paid_after.sum())))
        assert int(ws.max()) == res["env_steps"] <= MAX_STEPS
        assert ws.unique().numel() >= 2, (name, "every world ended at the same step")
        assert res["agents"] > 0
        seen |= out
        paid += int(paid_after.any())
    assert {OUTCOME_GOAL, OUTCOME_COLLISION, OUTCOME_TIMEOUT} <= seen, seen
    assert paid >= 1


@pytest.mark.parametrize("name", list(CASES))
def test_fused_crowd_round_equals_step_by_step(name):
    for spl in CASES[name][6]:
        _same_round(name, spl)


def test_sampled_evaluation():
    """greedy=False: the Philox draw of (seed, row, step counter + t) -- the same numbers as the step-by-step path draws, launch after launch"""
    name, spl = SAMPLED
    _same_round(name, spl, greedy=False)
    greedy, sampled = _reference(name)[0], _reference(name, greedy=False)[0]
    # (and the draw matters: the sampled round is not the greedy one)
    assert not torch.equal(greedy["per_agent"]["ret"], sampled["per_agent"]["ret"]) or greedy["env_steps"] != sampled["env_steps"]


def test_round_cut_at_max_steps():
    """max_steps = 10 with launches of 7: the last launch is cut to 3, and the round equals the step-by-step round cut at 10"""
    ROUNDS.cut_at_max_steps("n17_three_worlds")


def _raw(env, pol, rec, n, greedy=1, buffers=None):
    return tw.raw("cavoid_crowd_eval_run", env, pol, rec, n, greedy=greedy, buffers=buffers)


def test_launch_edges_at_the_raw_entry_point():
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords
    name = "n22_box"
    N, W = CASES[name][0], CASES[name][1]
    env, pol = _make(name)
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
    assert _raw(env, pol, rec, -1) == EINVAL
    other = _crowd_env(4, 20, 10, seed=3)                    # handles that do not describe the same batch: a policy of another width
    narrow = _policy(other.config, "free")
    assert _raw(env, narrow, rec, 4) == EINVAL
    narrow.close(); other.close()
    assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    # chunks of 7: after each, the running count is the world buffer's, and world_steps moved only in the worlds that were running
    rec.worlds_running.zero_()
    done_steps, counts = 0, []
    while done_steps < MAX_STEPS:
        was = _not_over(env)
        ws0 = rec.world_steps.clone()
        assert _raw(env, pol, rec, 7) == OK
        assert env.last_step_form == ("CROWD", 0)
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
    ref, _, log, _, _ = _reference(name)
    assert torch.equal(rec.world_steps, log.world_steps().to(rec.world_steps.device))
    assert torch.equal(rec.ret, log.masked_return(N)[0])
    pol.close(); env.close()


def test_last_step_form_reports_the_orca_form():
    """straight after the launch, with no cavoid_step in between (evaluate() settles the env with one)"""
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords
    for name, form in (("n20_orca", "CROWD_RVO"), ("n40_orca", "CROWD_RVO"), ("n33_m19", "CROWD")):
        env, pol = _make(name)
        env.reset()
        rec = _EvalRecords(env)
        assert _raw(env, pol, rec, 2) == OK
        assert env.last_step_form == (form, 0)
        assert int(rec.world_steps.max()) == 2
        pol.close(); env.close()


def test_policy_step_counter_advances_by_n_steps_per_launch():
    """the Philox draw reads the policy's step counter: after launches of 5 and 3 steps the handle draws what a handle draws after 8
    step-by-step calls -- and not what a fresh one draws"""
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords
    name = "n25_first_refill"
    env, a = _make(name)
    b, fresh = _policy(env.config, CASES[name][4]), _policy(env.config, CASES[name][4])
    obs = env.reset()
    x = obs.view(env.num_worlds * env.max_agents, -1)[:, 1:].clone()
    rec = _EvalRecords(env)
    assert _raw(env, a, rec, 5, greedy=0) == OK
    assert _raw(env, a, rec, 3, greedy=0) == OK
    for _ in range(8):
        b.act(x, greedy=False)
    draw = [p.act(x, greedy=False)[0].clone() for p in (a, b, fresh)]
    assert torch.equal(draw[0], draw[1])
    assert not torch.equal(draw[0], draw[2])
    for p in (a, b, fresh):
        p.close()
    env.close()


def test_the_entry_point_refuses_what_it_does_not_carry():
    """straight at the C ABI: the documented code, not a crash -- and the Python reason names the same thing"""
    from rl_collision_avoidance_amd.config import EnvConfig
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords, evaluate, evaluate_fused_crowd_unavailable_reason as why
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy

    def refused(code, word, env, pol):
        env.reset()
        rec = _EvalRecords(env)
        before = [t.clone() for t in (*env.get_state(), env.obs, rec.ret, rec.world_steps)]
        assert word in why(env, pol), why(env, pol)
        with pytest.raises(ValueError, match="fused_crowd=True"):
            evaluate(env, pol, fused_crowd=True)
        assert _raw(env, pol, rec, 4) == code
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) for u, v in zip(before, (*env.get_state(), env.obs, rec.ret, rec.world_steps)))
        pol.close(); env.close()

    env = _crowd_env(8, 16, 15, seed=1, evaluate_mode=1)                          # a tile env: cavoid_eval_run carries it
    refused(EUNSUPPORTED, "cavoid_eval_run", env, _policy(env.config, "free"))
    env = _crowd_env(8, 20, 7, seed=1, evaluate_mode=1)                           # a weight-sharing handle
    torch.manual_seed(1234)
    refused(EUNSUPPORTED, "weight_sharing", env, FusedPolicy(NetworkVP_rnn(env.config, arch="weight_sharing").to("cuda:0"), seed=77))
    env = _crowd_env(8, 20, 19, seed=1, evaluate_mode=1, dynamics=2)
    refused(EUNSUPPORTED, "holonomic", env, _policy(env.config, "free"))
    env = _crowd_env(8, 20, 19, seed=1, evaluate_mode=1, gen_min_agents=2, gen_nonlearning_fraction=0.5, gen_frozen_fraction=0.5)
    refused(EUNSUPPORTED, "frozen-network agents", env, _policy(env.config, "free"))
    # an unloaded handle: CAVOID_EINVAL (no FusedPolicy is ever unloaded: the raw handle)
    from rl_collision_avoidance_amd import _lib
    env = _crowd_env(8, 20, 19, seed=1, evaluate_mode=1)
    env.reset()
    rec = _EvalRecords(env)
    h = C.c_void_p()
    assert _lib.lib().cavoid_policy_create(19, 11, 0, C.byref(h)) == OK
    holder = type("Raw", (), {"_h": h})()
    assert _raw(env, holder, rec, 4) == EINVAL
    assert _raw(env, holder, rec, 0) == OK                   # (n_steps == 0 is answered first, as by cavoid_eval_run)
    _lib.lib().cavoid_policy_destroy(h)
    env.close()


_PRODUCTS_CHILD = """
import sys
sys.path.insert(0, %r)
import ctypes as C
import torch
from tests import test_gpu_crowd_eval as t
from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords, evaluate_fused_crowd_unavailable_reason as why
env, pol = t._make("n25_first_refill")
assert tuple(pol.inference_form) != ("split", 16), pol.inference_form
assert "non-default inference form" in why(env, pol)
env.reset()
rec = _EvalRecords(env)
assert t._raw(env, pol, rec, 4) == t.EUNSUPPORTED
torch.cuda.synchronize()
assert int(rec.world_steps.max()) == 0
print("REFUSED")
"""


def test_the_entry_point_refuses_a_non_default_product_form(tmp_path):
    """CAVOID_POLICY_PRODUCTS=3 is read at the handle's creation: a fresh child process"""
    script = tmp_path / "products3.py"
    script.write_text(_PRODUCTS_CHILD % ROOT)
    run = subprocess.run([sys.executable, str(script)], cwd=ROOT, env=dict(os.environ, CAVOID_POLICY_PRODUCTS="3"), timeout=300,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-3000:])
    assert run.returncode == 0 and run.stdout.strip().endswith("REFUSED")


def test_train_cli_runs_the_kernel_and_prints_the_same_result():
    fused, plain = tw.cli(["--agents", "20", "--worlds", "64", "--fused-crowd-evaluate"]), tw.cli(["--agents", "20", "--worlds", "64"])
    assert "[Evaluate] fused crowd evaluation kernel (cavoid_crowd_eval_run), 4 env steps per launch" in fused
    assert "cavoid_crowd_eval_run" not in plain
    last, strip = tw.last_evaluate_line, tw.without_mean_reward
    assert len(last(fused)) == 1 and len(last(plain)) == 1
    assert strip(last(fused)[0]) == strip(last(plain)[0])
    assert "success_rate" in strip(last(fused)[0]) and "mean_reward" not in strip(last(fused)[0])


def test_train_cli_with_the_flag_ends_where_the_kernel_does_not_apply():
    """with a reason the run ends with SystemExit naming it (in this process: nothing is evaluated before that)"""
    from rl_collision_avoidance_amd.ga3c import train
    with pytest.raises(SystemExit, match="--fused-crowd-evaluate.*cavoid_eval_run"):
        train.main(["--agents", "4", "--worlds", "64", "--evaluate", "1", "--fused-crowd-evaluate"])
    with pytest.raises(SystemExit, match="--fused-crowd-evaluate.*not a FusedPolicy"):
        train.main(["--agents", "20", "--worlds", "64", "--evaluate", "1", "--fused-crowd-evaluate", "--torch-policy"])
    tw.report_cache("crowd_eval")  # (a whole run of this file: 10 cases, the sampled round, the round cut at 10 steps: 12)
