"""GPU tests of the fused evaluation loop of crowd worlds with the weight_sharing network (`cavoid_crowd_eval_run_ws`,
csrc/cavoid_crowd_eval_ws.hpp; `ga3c.evaluate(fused_crowd_ws=True)`): whole EVALUATE_MODE rounds of worlds of 17..64 agents -- the ring form
of the weight_sharing pass on the tile's rows that still need an action, argmax (or the Philox draw), a second pass on a frozen network's
weights for the frozen-network agents, the crowd env.step without auto-reset, the outcome record, finished tiles leaving early -- in
launches of K env steps, against the same rounds driven step by step from the host (`evaluate()`: `policy.act` +
`frozen_policy.act(rows=...)` + `cavoid_step` + a look at the world buffer per step: code this kernel does not touch).  The kernel runs the
very same statements per value, so everything is compared BIT for bit: the result dict, every per-agent tensor, the world buffer the round
leaves behind, the records, and the observation the kernel left of the worlds that ended at the round's last step.  The pattern, the step
log and the comparison are tests/test_gpu_crowd_eval.py's.

The networks are `NetworkVP_rnn(arch="weight_sharing")` with their random initial weights and the bias of tests/test_gpu_eval_ws_fused.py on
one policy logit ("straight": full speed ahead, "turn": turning on the spot, "free": none); up to 19 observed neighbours they run on the
whole-row handle, above on the ring handle (`ws_crowd=True`).  The step-by-step result of every case is computed once and shared."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

from tests import eval_twins as tw
from tests.eval_twins import BIAS, MAX_STEPS, NETS, _not_over, _outcomes
from tests.gpu_support import EINVAL, EUNSUPPORTED, OK, _env as _crowd_env

pytestmark = pytest.mark.gpu

ORCA = dict(rvo_enabled=2, gen_rvo_fraction=0.5, gen_nonlearning_fraction=0.5)

# name: (N, W, M, env settings, network, max_time_ratio, steps per launch, frozen policy).  The shapes are the smallest at which the lane
# mapping, the row list, the ring or the recorder can go wrong.  Network and max_time_ratio are chosen per case, as
# tests/test_gpu_crowd_eval.py chose them, so that the STEP-BY-STEP round has what the case is compared on
# (test_the_step_by_step_rounds_are_not_empty); the reason stands beside each.
CASES = {
    # WS-8: three worlds per tile, 13 idle lanes, a ragged last tile, absent and scripted slots, M < N - 1, the whole-row handle.  "straight"
    # at the default ratio: sparse worlds (2..17 agents) are where agents of an untrained network reach goals
    "n17_ws8": (17, 50, 7, dict(sort_method="closest_first", gen_min_agents=2, gen_nonlearning_fraction=0.3), "straight", 1.75, (1, 7, 16), False),
    # M = R = 19: no slot of the ring is refilled.  "free", ratio 0.4: every world ends before the cut, by collisions and time-outs
    "n20_m19": (20, 24, 19, dict(), "free", 0.4, (16,), False),
    # R + 1: the ring's first refill, the ring handle.  "turn", ratio 0.4: nobody leaves its place, every agent runs out of time -- a world
    # ends by its slowest clock
    "n21_first_refill": (21, 24, 20, dict(), "turn", 0.4, (7,), False),
    # two worlds per tile, box scenarios generated in the step.  "free", ratio 0.5: a short round of collisions and time-outs, and the loop
    # pays agents that ran out of time beside another after their world's end (the two definitions of the return differ)
    "n22_box": (22, 33, 21, dict(gen_mode=1, gen_pool_size=0), "free", 0.5, (7,), False),
    # one world per tile, 31 idle lanes.  "straight", ratio 0.5: collisions and time-outs
    "n33_one_world": (33, 20, 32, dict(sort_method="closest_last"), "straight", 0.5, (7,), False),
    # above 2 R: a slot refilled twice.  "straight", ratio 0.4: collisions and time-outs
    "n48_two_refills": (48, 10, 47, dict(), "straight", 0.4, (7,), False),
    # all 64 lanes, the full-width world mask, absent slots.  "straight" at the default ratio: goals in the sparse worlds
    "n64_full_mask": (64, 12, 63, dict(gen_min_agents=2), "straight", 1.75, (16,), False),
    # ORCA agents, both buckets (the <32, true, false> and <64, true, false> instantiations).  "free" / "straight", ratio 0.5: half the
    # agents are scripted and go on being paid by the loop after their world's end
    "n20_orca": (20, 30, 19, dict(ORCA), "free", 0.5, (7,), False),
    "n40_orca": (40, 12, 39, dict(ORCA), "straight", 0.5, (16,), False),
    # 520 workgroups: two per CU on every CU.  "turn", ratio 0.2: a short round that still ends worlds at many different steps
    "n33_two_per_cu": (33, 520, 7, dict(), "turn", 0.2, (16,), False),
    # frozen-network agents and a second weight_sharing network for them on the whole-row handle (<32, false, true>).  "free", ratio 0.5:
    # half the agents are scripted, and the static share (0.5 by default) leaves the other half of those to the frozen network
    "n20_frozen": (20, 30, 19, dict(gen_frozen_fraction=0.5, gen_nonlearning_fraction=0.5), "free", 0.5, (7,), True),
    # ORCA agents AND frozen-network agents, the frozen network on the ring handle (<64, true, true>).  "straight", ratio 0.5.  The static
    # share is cut to 0.1: at its default of 0.5 the ORCA share of 0.5 leaves the draw no room for a frozen-network agent
    "n40_orca_frozen": (40, 12, 39, dict(ORCA, gen_static_fraction=0.1, gen_frozen_fraction=0.3), "straight", 0.5, (16,), True),
}
SAMPLED = ("n22_box", 7)             # the sampled case: greedy=False on this shape, one round


def _policy(cfg, net, seed=1234, policy_seed=77, arch="weight_sharing"):
    # the whole-row handle up to 19 observed neighbours, the ring handle above
    return tw.policy(cfg, net, seed, policy_seed, arch, ws_crowd=None)


def _make(name, **more):
    N, W, M, over, net, ratio, _, frozen = CASES[name]
    env = _crowd_env(W, N, M, seed=21, evaluate_mode=1, max_time_ratio=ratio, **dict(over, **more))
    pol = _policy(env.config, net)
    fz = _policy(env.config, "free", seed=4321, policy_seed=0) if frozen else None
    assert pol.ws and pol.crowd == (M > 19) and (fz is None or fz.crowd == (M > 19))
    return env, pol, fz


_close = tw.close


def _frozen_rows(env, name):
    """per step of the step-by-step round, the number of running frozen-network rows the loop listed"""
    from rl_collision_avoidance_amd import _lib
    frozen_rows, rows_of = [], env.policy_rows

    def spy(policy_id, only_running=True):
        out = rows_of(policy_id, only_running)
        if policy_id == _lib.POLICY_FROZEN_NET:
            frozen_rows.append(int(out[1].item()))
        return out
    return spy, frozen_rows


# the step-by-step round of every case is computed once (family "crowd_ws_eval" of the one cache)
ROUNDS = tw.CrowdRounds("crowd_ws_eval", CASES, lambda name: _make(name), switch="fused_crowd_ws",
                        reason="evaluate_fused_crowd_ws_unavailable_reason", run="eval_run_crowd_ws", rows_spy=_frozen_rows)
_reference, _same_round = ROUNDS.reference, ROUNDS.same_round


def test_the_step_by_step_rounds_are_not_empty():
    """Conditions on the STEP-BY-STEP side (code of before), so that no comparison below passes on nothing: every case ends its worlds at
    two or more different steps (early exit happened) and has learning agents, the cases together see every outcome, in at least one the
    loop paid an agent after its world was over (the two definitions of the return differ), every frozen case listed running
    frozen-network rows at one step at least, and every ring case (M >= 20) had a live row: at a round's first step every learning agent
    is one, so learning agents and one step taken say so."""
    from rl_collision_avoidance_amd.ga3c.evaluate import OUTCOME_COLLISION, OUTCOME_GOAL, OUTCOME_TIMEOUT
    seen, paid = set(), 0
    for name, (N, W, M, over, net, ratio, _, frozen) in CASES.items():
        res, state, log, _, frozen_rows = _reference(name)
        ws = log.world_steps()
        masked, paid_after = log.masked_return(N)
        out = _outcomes(res)
        print("%-18s N %2d W %3d M %2d %-8s ratio %.2f: env_steps %3d world_steps min %3d median %3d distinct %2d outcomes %s learning %d paid after %d "
              "frozen rows max %d" % (name, N, W, M, net, ratio, res["env_steps"], int(ws.min()), int(ws.median()), ws.unique().numel(), sorted(out),
                                      res["agents"], int(paid_after.sum()), max(frozen_rows) if frozen_rows else 0))
        assert int(ws.max()) == res["env_steps"] <= MAX_STEPS
        assert ws.unique().numel() >= 2, (name, "every world ended at the same step")
        assert res["agents"] > 0 and res["env_steps"] >= 1
        if frozen:
            assert len(frozen_rows) == res["env_steps"] and max(frozen_rows) > 0, (name, "no running frozen-network agent at any step")
        else:
            assert not frozen_rows
        seen |= out
        paid += int(paid_after.any())
    assert {OUTCOME_GOAL, OUTCOME_COLLISION, OUTCOME_TIMEOUT} <= seen, seen
    assert paid >= 1


@pytest.mark.parametrize("name", list(CASES))
def test_fused_crowd_ws_round_equals_step_by_step(name):
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
    """max_steps = 10 with launches of 7: the last launch is cut to 3 (the cut lies inside a launch of the uncut round), and the round
    equals the step-by-step round cut at 10"""
    ROUNDS.cut_at_max_steps("n17_ws8")


def _raw(env, pol, rec, n, frozen=None, greedy=1, buffers=None):
    return tw.raw("cavoid_crowd_eval_run_ws", env, pol, rec, n, frozen, greedy, buffers)


def test_launch_edges_at_the_raw_entry_point():
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords
    name = "n22_box"
    N, W = CASES[name][0], CASES[name][1]
    env, pol, _ = _make(name)
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
    # a second chain of launches on worlds that are all over: no byte of obs, the state or the records changes, nobody running
    before = snap()
    for n in (16, 7, 1):
        rec.worlds_running.fill_(5)
        assert _raw(env, pol, rec, n) == OK
        assert int(rec.worlds_running.item()) == 0
        after = snap()
        assert all(torch.equal(a, b) for a, b in zip(before[:7], after[:7])) and torch.equal(before[8], after[8])   # ([7]: the running count)
    # the records are the step-by-step round's
    ref, _, log, _, _ = _reference(name)
    assert torch.equal(rec.world_steps, log.world_steps().to(rec.world_steps.device))
    assert torch.equal(rec.ret, log.masked_return(N)[0])
    _close(env, pol, None)


def test_last_step_form_reports_the_orca_form():
    """straight after the launch, with no cavoid_step in between (evaluate() settles the env with one)"""
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords
    for name, form in (("n20_orca", "CROWD_RVO"), ("n40_orca_frozen", "CROWD_RVO"), ("n33_one_world", "CROWD"), ("n20_frozen", "CROWD")):
        env, pol, fz = _make(name)
        env.reset()
        rec = _EvalRecords(env)
        assert _raw(env, pol, rec, 2, frozen=fz) == OK
        assert env.last_step_form == (form, 0)
        assert int(rec.world_steps.max()) == 2
        _close(env, pol, fz)


def test_policy_step_counter_advances_by_n_steps_per_launch():
    """the Philox draw reads the policy's step counter: after launches of 5 and 3 steps the handle draws what a handle draws after 8
    step-by-step calls -- and not what a fresh one draws"""
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords
    name = "n21_first_refill"
    env, a, _ = _make(name)
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
    """straight at the C ABI: the documented code, not a crash, nothing written -- and the Python reason names the same thing"""
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords, evaluate, evaluate_fused_crowd_ws_unavailable_reason as why

    def refused(code, word, env, pol, fz=None):
        env.reset()
        rec = _EvalRecords(env)
        before = [t.clone() for t in (*env.get_state(), env.obs, rec.ret, rec.world_steps)]
        assert word in why(env, pol, fz), why(env, pol, fz)
        with pytest.raises(ValueError, match="fused_crowd_ws=True"):
            evaluate(env, pol, frozen_policy=fz, fused_crowd_ws=True)
        assert _raw(env, pol, rec, 4, frozen=fz) == code
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) for u, v in zip(before, (*env.get_state(), env.obs, rec.ret, rec.world_steps)))
        _close(env, pol, fz)

    env = _crowd_env(8, 20, 19, seed=1, evaluate_mode=1)                          # an LSTM handle: cavoid_crowd_eval_run carries it
    refused(EUNSUPPORTED, "cavoid_crowd_eval_run", env, _policy(env.config, "free", arch="rnn"))
    env = _crowd_env(8, 16, 7, seed=1, evaluate_mode=1)                           # a tile env: cavoid_eval_run_ws carries it
    refused(EUNSUPPORTED, "cavoid_eval_run_ws", env, _policy(env.config, "free"))
    env = _crowd_env(8, 20, 19, seed=1, evaluate_mode=1, dynamics=2)
    refused(EUNSUPPORTED, "holonomic", env, _policy(env.config, "free"))
    env = _crowd_env(8, 20, 19, seed=1, evaluate_mode=1)                          # a frozen handle of another max_other
    other = _crowd_env(1, 20, 7, seed=1, evaluate_mode=1)
    narrow = _policy(other.config, "free")
    other.close()
    refused(EUNSUPPORTED, "frozen policy", env, _policy(env.config, "free"), narrow)
    env = _crowd_env(8, 20, 19, seed=1, evaluate_mode=1)                          # ... and an LSTM frozen handle
    refused(EUNSUPPORTED, "frozen policy", env, _policy(env.config, "free"), _policy(env.config, "free", arch="rnn"))
    env = _crowd_env(8, 20, 19, seed=1, evaluate_mode=1, gen_min_agents=2, gen_nonlearning_fraction=0.5, gen_frozen_fraction=0.5)
    refused(EUNSUPPORTED, "frozen-network agents", env, _policy(env.config, "free"))      # a frozen-generating env with frozen = NULL
    env = _crowd_env(8, 20, 19, seed=1, evaluate_mode=1)                          # mismatching max_other: the handles describe other batches
    other = _crowd_env(1, 20, 7, seed=1, evaluate_mode=1)
    narrow = _policy(other.config, "free")
    other.close()
    refused(EINVAL, "neighbours", env, narrow)
    # an unloaded handle: CAVOID_EINVAL (no FusedPolicy is ever unloaded: the raw handle)
    env = _crowd_env(8, 20, 19, seed=1, evaluate_mode=1)
    env.reset()
    rec = _EvalRecords(env)
    h = C.c_void_p()
    assert _lib.lib().cavoid_policy_create_ws(19, 11, 0, C.byref(h)) == OK
    holder = type("Raw", (), {"_h": h})()
    assert _raw(env, holder, rec, 4) == EINVAL
    assert _raw(env, holder, rec, 0) == OK                   # (n_steps == 0 is answered first, as by cavoid_eval_run)
    loaded = _policy(env.config, "free")
    assert _raw(env, loaded, rec, 4, frozen=holder) == EINVAL                     # ... and an unloaded frozen handle
    torch.cuda.synchronize()
    assert int(rec.world_steps.max()) == 0
    _lib.lib().cavoid_policy_destroy(h)
    loaded.close(); env.close()


def test_the_other_switches_keep_their_reasons_on_these_envs_and_policies():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate
    for name in ("n17_ws8", "n21_first_refill"):
        env, pol, _ = _make(name)
        with pytest.raises(ValueError, match=r"fused_crowd=True\) does not apply: the policy is the weight_sharing network \(the crowd evaluation "
                                             r"kernel embeds the LSTM pass; the weight_sharing ring form is evaluated step by step\)"):
            evaluate(env, pol, fused_crowd=True)
        old = ("crowd worlds \\(more than 16\\) are evaluated step by step" if name == "n17_ws8"
               else "neighbours on the ring kernels \\(the weight_sharing evaluation kernel parks the whole row")
        with pytest.raises(ValueError, match=r"fused_ws=True\) does not apply: .*" + old):
            evaluate(env, pol, fused_ws=True)
        with pytest.raises(ValueError, match=r"fused=True\) does not apply: .*crowd worlds \(more than 16\) are evaluated step by step"):
            evaluate(env, pol, fused=True)
        _close(env, pol, None)


def test_train_cli_runs_the_kernel_and_prints_the_same_result(tmp_path):
    """a fresh child process each, on a checkpoint this test writes (a weight_sharing network of 19 observed neighbours, "straight")"""
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    env = _crowd_env(1, 20, 19, seed=1)
    net = NetworkVP_rnn(env.config, seed=1234, arch="weight_sharing")
    env.close()
    with torch.no_grad():
        net.p_bias[NETS["straight"]] += BIAS
    ckpt = str(tmp_path / "network_00000000.pt")
    torch.save({"episode": 0, "model": net.state_dict(), "training_step": 0, "arch": net.arch, "max_others": net.max_others}, ckpt)
    args = ["--arch", "weight_sharing", "--agents", "20", "--observed", "19", "--worlds", "24", "--load", ckpt]
    fused, plain = tw.cli(args + ["--fused-crowd-ws-evaluate"]), tw.cli(args)
    assert "[Evaluate] fused crowd weight_sharing evaluation kernel (cavoid_crowd_eval_run_ws), 4 env steps per launch" in fused
    assert "cavoid_crowd_eval_run_ws" not in plain
    last, strip = tw.last_evaluate_line, tw.without_mean_reward
    assert len(last(fused)) == 1 and len(last(plain)) == 1
    assert strip(last(fused)[0]) == strip(last(plain)[0])
    assert "success_rate" in strip(last(fused)[0]) and "mean_reward" not in strip(last(fused)[0])


def test_train_cli_with_the_flag_ends_where_the_kernel_does_not_apply():
    """with a reason the run ends with SystemExit naming it (in this process: nothing is evaluated before that)"""
    from rl_collision_avoidance_amd.ga3c import train
    with pytest.raises(SystemExit, match="--fused-crowd-ws-evaluate.*cavoid_eval_run_ws"):
        train.main(["--agents", "4", "--worlds", "64", "--arch", "weight_sharing", "--evaluate", "1", "--fused-crowd-ws-evaluate"])
    with pytest.raises(SystemExit, match="--fused-crowd-ws-evaluate.*cavoid_crowd_eval_run embeds"):
        train.main(["--agents", "20", "--worlds", "64", "--evaluate", "1", "--fused-crowd-ws-evaluate"])
    tw.report_cache("crowd_ws_eval")  # (a whole run of this file: 12 cases, the sampled round, the round cut at 10 steps: 14)
