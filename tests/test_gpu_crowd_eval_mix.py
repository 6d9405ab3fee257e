"""GPU tests of the fused evaluation loop of crowd worlds with frozen-network agents (`cavoid_crowd_eval_run_mix`,
csrc/cavoid_crowd_eval_mix.hpp: `crowd_mix_evaluate_kernel<NB, RVO>`; `ga3c.evaluate(fused_crowd_mix=True)`): whole EVALUATE_MODE rounds of
worlds of 17..64 agents -- the ring form of the policy pass, the same pass once more on a second, frozen network for the tile's running
frozen-network agents, argmax (or the Philox draw), the crowd env.step without auto-reset, the outcome record, finished tiles leaving early
-- in launches of K env steps, against the same rounds driven step by step from the host (`evaluate(frozen_policy=...)`: `policy.act` +
`frozen_policy.act(rows=...)` + `cavoid_step` + a look at the world buffer per step: code this kernel does not touch).  The kernel runs the
very same statements per value, so everything is compared BIT for bit: the result dict, every per-agent tensor, the world buffer the round
leaves behind, the records, and the observation the kernel left of the worlds that ended at the round's last step; the return under the two
definitions the README states (tests/test_gpu_eval_fused.py's `_assert_same`).  The pattern is tests/test_gpu_crowd_eval.py's.

The step-by-step result of every case is computed once and shared; with it, per step, the host notes from the world buffer's flags which
tiles had no learner row left that needs an action but a running frozen-network row: the steps at which the kernel runs the frozen pass
alone."""
import pytest

torch = pytest.importorskip("torch")

from tests import eval_twins as tw
from tests.eval_twins import MAX_STEPS, policy as _policy
from tests.gpu_support import EINVAL, EUNSUPPORTED, OK, _env as _crowd_env

pytestmark = pytest.mark.gpu

MIX = dict(gen_nonlearning_fraction=0.5, gen_frozen_fraction=0.5)            # (with the default static share: about a quarter frozen-network agents)
# ORCA agents AND frozen-network agents: the settings of tests/test_gpu_crowd_ws_eval.py (the default static share leaves no room for them)
ORCA_MIX = dict(rvo_enabled=2, gen_rvo_fraction=0.5, gen_static_fraction=0.1, gen_frozen_fraction=0.3, gen_nonlearning_fraction=0.5)

# name: (N, W, M, env settings, network, max_time_ratio, steps per launch).  Short rounds (every agent runs out of time unless it collides
# first): the time ratio only sets how long the round is, and an agent's clock runs by its own distance to its goal, so a frozen-network
# agent with a long way outlasts the learners of its tile.
CASES = {
    "n20": (20, 30, 19, dict(MIX), "free", 0.4, 7),                    # three worlds per tile, no ring refill
    "n25_first_refill": (25, 21, 24, dict(MIX), "turn", 0.3, 1),        # the first ring refill on both handles; one step per launch
    "n33_one_world": (33, 20, 32, dict(MIX), "straight", 0.4, 16),      # one world per tile
    "n40_orca": (40, 12, 39, dict(ORCA_MIX), "straight", 0.4, 16),      # ORCA + frozen (<64, true>)
    "n64_full_mask": (64, 8, 63, dict(MIX), "free", 0.3, 7),            # all 64 lanes
}
SAMPLED = "n20"


def _make(name):
    N, W, M, over, net, ratio, _ = CASES[name]
    env = _crowd_env(W, N, M, seed=21, evaluate_mode=1, max_time_ratio=ratio, **over)
    return env, _policy(env.config, net), _policy(env.config, "free", seed=4321, policy_seed=0)


_close = tw.close


def _frozen_pass_alone(env, name):
    """per step of the step-by-step round: (frozen rows listed, tiles with a running frozen-network row and no learner row that needs an
    action), noted from the world buffer's flags BEFORE the step"""
    from rl_collision_avoidance_amd import _lib
    N, W = CASES[name][0], CASES[name][1]
    per_step, rows_of = [], env.policy_rows
    wpw = 64 // N
    tiles = (W + wpw - 1) // wpw

    def spy(policy_id, only_running=True):
        out = rows_of(policy_id, only_running)
        if policy_id == _lib.POLICY_FROZEN_NET:
            fl = env.get_state()[2].view(-1).long()                                  # the state BEFORE this step
            live = ((fl & _lib.F_PRESENT) != 0) & ((fl & _lib.F_LEARNING) != 0) & ((fl & _lib.F_DONE_MASK) == 0)
            frozen = torch.zeros_like(live)
            frozen[out[0][:int(out[1].item())].long()] = True
            pol4 = ((fl >> _lib.F_POLICY_SHIFT) & _lib.F_POLICY_MASK) == _lib.POLICY_FROZEN_NET
            assert bool((frozen == (pol4 & ((fl & _lib.F_PRESENT) != 0) & ((fl & _lib.F_DONE_MASK) == 0))).all())   # (the kernel's predicate)
            pad = tiles * wpw * N - W * N
            tile = lambda m: torch.cat([m, m.new_zeros(pad)]).view(tiles, wpw * N).any(1)
            per_step.append((int(frozen.sum()), int((tile(frozen) & ~tile(live)).sum())))
        return out
    return spy, per_step


def _one_network_switch_refuses(ev, env, pol, fz):
    assert "frozen_policy" in ev.evaluate_fused_crowd_unavailable_reason(env, pol, fz)   # (the one-network switch goes on refusing)


# the step-by-step round of every case is computed once (family "crowd_eval_mix" of the one cache)
ROUNDS = tw.CrowdRounds("crowd_eval_mix", CASES, lambda name: _make(name), switch="fused_crowd_mix",
                        reason="evaluate_fused_crowd_mix_unavailable_reason", run="eval_run_crowd_mix", rows_spy=_frozen_pass_alone,
                        also=_one_network_switch_refuses)
_reference, _same_round = ROUNDS.reference, ROUNDS.same_round


def test_the_step_by_step_rounds_show_the_frozen_pass_and_the_frozen_pass_alone():
    """Conditions on the STEP-BY-STEP side (code of before), so that no comparison below passes on nothing: every case lists running
    frozen-network rows, ends its worlds at different steps (early exit happened) within the cut, and at least one case has steps at which a
    tile holds a running frozen-network row and no learner row that needs an action -- the kernel's 'frozen pass alone' branch."""
    alone_cases = 0
    for name, (N, W, M, over, net, ratio, spl) in CASES.items():
        res, _, log, _, per_step = _reference(name)
        ws = log.world_steps()
        listed = sum(1 for f, _ in per_step if f > 0)
        alone = sum(a for _, a in per_step)
        print("%-18s N %2d W %3d M %2d %-8s ratio %.2f: env_steps %3d world_steps min %3d distinct %2d learning %d; frozen rows listed at %d steps "
              "(max %d), (step, tile) pairs with the frozen pass alone: %d" % (name, N, W, M, net, ratio, res["env_steps"], int(ws.min()),
                                                                               ws.unique().numel(), res["agents"], listed,
                                                                               max(f for f, _ in per_step), alone))
        assert len(per_step) == res["env_steps"] == int(ws.max()) <= MAX_STEPS
        assert ws.unique().numel() >= 2, (name, "every world ended at the same step")
        assert res["agents"] > 0 and listed > 0
        alone_cases += int(alone > 0)
    assert alone_cases >= 1


@pytest.mark.parametrize("name", list(CASES))
def test_fused_crowd_mix_round_equals_step_by_step(name):
    _same_round(name, CASES[name][6])


def test_sampled_evaluation():
    """greedy=False: the learner's rows take the Philox draw of (seed, row, step counter + t), the frozen rows still the argmax"""
    _same_round(SAMPLED, CASES[SAMPLED][6], greedy=False)
    greedy, sampled = _reference(SAMPLED)[0], _reference(SAMPLED, greedy=False)[0]
    assert not torch.equal(greedy["per_agent"]["ret"], sampled["per_agent"]["ret"]) or greedy["env_steps"] != sampled["env_steps"]


def test_round_cut_at_max_steps():
    """max_steps = 10 with launches of 7: the last launch is cut to 3, and the round equals the step-by-step round cut at 10"""
    ROUNDS.cut_at_max_steps("n20")


def _raw(env, pol, fz, rec, n, greedy=1):
    return tw.raw("cavoid_crowd_eval_run_mix", env, pol, rec, n, fz, greedy)


def test_launch_edges_at_the_raw_entry_point():
    """n_steps == 0, null arguments, and a launch on finished worlds: nothing changes and worlds_running is 0"""
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords
    name = "n20"
    N = CASES[name][0]
    env, pol, fz = _make(name)
    env.reset()
    rec = _EvalRecords(env)
    snap = lambda: [t.clone() for t in (*env.get_state(), env.obs, rec.ret, rec.goal_step, rec.world_steps, rec.worlds_running, rec.actions)]
    rec.worlds_running.fill_(-7)
    before = snap()
    assert _raw(env, pol, fz, rec, 0) == OK                   # n_steps == 0: OK, nothing touched (not even the running count)
    assert _raw(env, pol, None, rec, 0) == EINVAL             # `frozen` is required: refused before n_steps == 0 is looked at
    assert _raw(env, None, fz, rec, 4) == EINVAL
    assert _raw(env, pol, fz, rec, -1) == EINVAL
    assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    rec.worlds_running.zero_()
    steps = 0
    while steps < MAX_STEPS:
        assert _raw(env, pol, fz, rec, 16) == OK
        assert env.last_step_form == ("CROWD", 0)
        steps += 16
        if int(rec.worlds_running.item()) == 0:
            break
    assert int(rec.worlds_running.item()) == 0
    # a launch on worlds that are all over: state, records and obs unchanged, nobody running
    before = snap()
    assert _raw(env, pol, fz, rec, 16) == OK
    assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    assert int(rec.worlds_running.item()) == 0
    # the records are the step-by-step round's
    _, _, log, _, _ = _reference(name)
    assert torch.equal(rec.world_steps, log.world_steps().to(rec.world_steps.device))
    assert torch.equal(rec.ret, log.masked_return(N)[0])
    _close(env, pol, fz)


def test_the_entry_point_refuses_what_it_does_not_carry():
    """straight at the C ABI: the documented code, not a crash -- and the Python reason names the same thing"""
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords, evaluate, evaluate_fused_crowd_mix_unavailable_reason as why
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy

    def refused(code, word, env, pol, fz):
        env.reset()
        rec = _EvalRecords(env)
        before = [t.clone() for t in (*env.get_state(), env.obs, rec.ret, rec.world_steps)]
        assert word in why(env, pol, fz), why(env, pol, fz)
        with pytest.raises(ValueError, match="fused_crowd_mix=True"):
            evaluate(env, pol, frozen_policy=fz, fused_crowd_mix=True)
        assert _raw(env, pol, fz, rec, 4) == code
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) for u, v in zip(before, (*env.get_state(), env.obs, rec.ret, rec.world_steps)))
        pol.close(); env.close()
        if fz is not None:
            fz.close()

    ws = lambda cfg: FusedPolicy(NetworkVP_rnn(cfg, seed=1234, arch="weight_sharing").to("cuda:0"), seed=77)
    env = _crowd_env(8, 16, 15, seed=1, evaluate_mode=1, **MIX)                   # a tile env: cavoid_eval_run carries it
    refused(EUNSUPPORTED, "cavoid_eval_run", env, _policy(env.config, "free"), _policy(env.config, "free", seed=4321))
    env = _crowd_env(8, 20, 7, seed=1, evaluate_mode=1, **MIX)                    # a weight-sharing policy
    refused(EUNSUPPORTED, "weight_sharing", env, ws(env.config), _policy(env.config, "free", seed=4321))
    env = _crowd_env(8, 20, 7, seed=1, evaluate_mode=1, **MIX)                    # a weight-sharing frozen policy
    refused(EUNSUPPORTED, "frozen policy is the weight_sharing network", env, _policy(env.config, "free"), ws(env.config))
    env = _crowd_env(8, 20, 19, seed=1, evaluate_mode=1, **MIX)                   # a frozen policy of fewer neighbours
    other = _crowd_env(4, 20, 10, seed=3)
    refused(EUNSUPPORTED, "frozen policy observes 10 neighbours", env, _policy(env.config, "free"), _policy(other.config, "free", seed=4321))
    other.close()
    env = _crowd_env(8, 20, 19, seed=1, evaluate_mode=1, dynamics=2, **MIX)
    refused(EUNSUPPORTED, "holonomic", env, _policy(env.config, "free"), _policy(env.config, "free", seed=4321))
    env = _crowd_env(8, 20, 19, seed=1, evaluate_mode=1, **MIX)                   # no frozen_policy
    refused(EINVAL, "no frozen_policy", env, _policy(env.config, "free"), None)
    tw.report_cache("crowd_eval_mix")  # (a whole run of this file: 5 cases, the sampled round, the round cut at 10 steps: 7)
