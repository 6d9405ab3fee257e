"""GPU tests of the fused evaluation loop of the weight-sharing network (`cavoid_eval_run_ws`, csrc/cavoid_eval_ws.hpp;
`ga3c.evaluate(fused_ws=True)`): whole EVALUATE_MODE rounds -- the weight-sharing pass, argmax (or the Philox draw), env.step without
auto-reset, outcome record, finished tiles leaving early -- in launches of K env steps, against the same rounds driven step by step from the
host (`evaluate(fused=False)`: `cavoid_policy_forward` on the weight-sharing handle + `cavoid_step` + a look at the world buffer per step).
The kernel runs the very same statements per value, so everything is compared BIT for bit: the result dict, every per-agent tensor, the
world buffer the round leaves behind, and the return against its definition (include/cavoid.h) via the step log.

The networks are `NetworkVP_rnn(arch="weight_sharing")` with their random initial weights and a bias on one policy logit (the helpers and
the three behaviours of tests/test_gpu_eval_fused.py).  The step-by-step result of every (shape, network) is computed once and shared."""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")

from tests import eval_twins as tw
from tests.eval_twins import MAX_STEPS, MIX, NETS, SPLS, _assert_same, _not_over, _outcomes, _StepLog
from tests.gpu_support import EINVAL, EUNSUPPORTED, OK, ROOT, _env as _crowd_env

pytestmark = pytest.mark.gpu

FAMILY = "eval_ws_fused"         # this file's rounds in the one cache of step-by-step references


def _cfg(N, M):
    from rl_collision_avoidance_amd.config import EnvConfig

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = M
            EnvConfig.__init__(self)
    return Cfg()


def _policy(cfg, net, seed=1234, policy_seed=77, arch="weight_sharing", ws_crowd=False):
    return tw.policy(cfg, net, seed, policy_seed, arch, ws_crowd)


def _env(W, N, M, seed, **over):
    over.setdefault("evaluate_mode", 1)
    over.setdefault("max_time_ratio", 1.75)
    return _crowd_env(W, N, M, seed=seed, **over)


def _make(W, N, M, net, frozen, over):
    env = _env(W, N, M, 21, **over)
    pol = _policy(env.config, net)
    fz = _policy(env.config, "free", seed=4321, policy_seed=0) if frozen else None
    return env, pol, fz


_close = tw.close


def _reference(W, N, M, net, greedy=True, frozen=False, **over):
    """evaluate(fused=False, details=True) of one (shape, network): result, final world buffer, the step log -- computed once"""
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate

    def compute():
        env, pol, fz = _make(W, N, M, net, frozen, over)
        log = _StepLog(env)
        res = evaluate(env, pol, rounds=1, greedy=greedy, max_steps=MAX_STEPS, frozen_policy=fz, details=True)
        out = (res, [t.clone() for t in env.get_state()], log)
        _close(env, pol, fz)
        return out
    return tw.cached(FAMILY, (W, N, M, net, greedy, frozen, tuple(sorted(over.items()))), compute)


def _fused(W, N, M, net, spl, greedy=True, frozen=False, **over):
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate, evaluate_fused_ws_unavailable_reason
    env, pol, fz = _make(W, N, M, net, frozen, over)
    assert evaluate_fused_ws_unavailable_reason(env, pol, fz) is None         # (no case passes by falling back: fused_ws=True would raise, too)
    res = evaluate(env, pol, rounds=1, greedy=greedy, max_steps=MAX_STEPS, frozen_policy=fz, fused_ws=True, steps_per_launch=spl, details=True)
    state = [t.clone() for t in env.get_state()]
    _close(env, pol, fz)
    return res, state


def _report(W, N, M, net, res, log):
    ws = log.world_steps()
    assert int(ws.max()) == res["env_steps"] <= MAX_STEPS
    print("%dx%d M=%d %-8s env_steps %d world_steps min %d median %d distinct %d outcomes %s" % (
        N, W, M, net, res["env_steps"], int(ws.min()), int(ws.median()), ws.unique().numel(), sorted(_outcomes(res))))
    return ws


SHAPES = {                                                  # W, N, M, env overrides
    "ws8": (64, 4, 7, dict()),                              # WS-8: slots past the neighbour count, the cooperative (quad) env step
    "ws8_closest_first": (64, 4, 7, dict(sort_method=1)),  # the WS baselines' order
    "n4_ragged": (13, 4, 7, dict()),                        # one ragged tile (13 of 16 worlds)
    "n5_2to5_present": (60, 5, 4, dict(gen_min_agents=2)),  # absent slots
    "n6_clip": (40, 6, 3, dict()),                          # M < N - 1: the observation clips to the M nearest
    "n10_box_widest_row": (24, 10, 19, dict(gen_mode=1)),  # the widest parked row, single-wavefront env step, box scenarios (the ORCA instantiation's route)
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_round_equals_step_by_step(shape):
    W, N, M, over = SHAPES[shape]
    for net in NETS:
        ref, ref_state, log = _reference(W, N, M, net, **over)
        _report(W, N, M, net, ref, log)
        for spl in SPLS:
            got, got_state = _fused(W, N, M, net, spl, **over)
            _assert_same(ref, ref_state, got, got_state, (shape, net, spl), log)


def test_references_are_not_empty_of_what_early_exit_is_about():
    """tests/test_gpu_eval_fused.py's `_check_not_empty` on the weight-sharing references of the WS-8 shape: early exit happened, and the
    three networks together saw every outcome"""
    from rl_collision_avoidance_amd.ga3c.evaluate import OUTCOME_COLLISION, OUTCOME_GOAL, OUTCOME_TIMEOUT
    W, N, M, over = SHAPES["ws8"]
    seen, spread = set(), False
    for net in NETS:
        res, _, log = _reference(W, N, M, net, **over)
        seen |= _outcomes(res)
        ws = _report(W, N, M, net, res, log)
        if ws.unique().numel() >= 3 and 2 * int(ws.min()) < int(ws.max()):
            spread = True
        if net == "straight":      # the network that ends worlds early: its round must show the spread early exit is about
            assert ws.unique().numel() >= 3 and 2 * int(ws.min()) < int(ws.max()), (ws.unique().tolist())
    assert spread
    assert {OUTCOME_GOAL, OUTCOME_COLLISION, OUTCOME_TIMEOUT} <= seen, seen


def test_sixteen_agents_at_the_widest_row_the_kernel_takes():
    """16 x 32 at the widest M the reason function lets through -- which is the parked row's limit, 19: without ORCA lines the env step's
    LDS fits the lent rows at every width"""
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate_fused_ws_unavailable_reason as why
    cfg = SimpleNamespace(dynamics=0, gen_frozen_fraction=0.0, gen_nonlearning_fraction=0.0, rvo_enabled=0)
    pol = lambda m: SimpleNamespace(act=None, inference_form=("f32", 0), _h=object(), arch="weight_sharing", ws=True, crowd=m > 19, max_others=m,
                                    num_actions=11)
    fits = [m for m in range(1, 65) if why(SimpleNamespace(max_agents=16, max_other=m, cfg=cfg), pol(m)) is None]
    assert fits == list(range(1, 20)), fits
    M = fits[-1]
    for net in ("straight", "free"):
        ref, ref_state, log = _reference(32, 16, M, net)
        _report(32, 16, M, net, ref, log)
        for spl in SPLS:
            got, got_state = _fused(32, 16, M, net, spl)
            _assert_same(ref, ref_state, got, got_state, ("n16", M, net, spl), log)


_CHILD = """
import sys
sys.path.insert(0, %r)
from tests import test_gpu_eval_ws_fused as t
W, N, M, over = t.SHAPES["ws8"]
for net in t.NETS:
    ref, ref_state, log = t._reference(W, N, M, net, **over)
    for spl in t.SPLS:
        got, got_state = t._fused(W, N, M, net, spl, **over)
        t._assert_same(ref, ref_state, got, got_state, (net, spl), log)
print("SAME")
"""


def test_fused_round_equals_step_by_step_on_one_wavefront(tmp_path):
    """WS-8 with CAVOID_ACTOR_QUAD=0 (read at the launch): the tile's env step by wavefront 0 alone, in a child process"""
    script = tmp_path / "quad0.py"
    script.write_text(_CHILD % ROOT)
    run = subprocess.run([sys.executable, str(script)], cwd=ROOT, env=dict(os.environ, CAVOID_ACTOR_QUAD="0"), timeout=300,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-3000:])
    assert run.returncode == 0 and run.stdout.strip().endswith("SAME")


@pytest.mark.parametrize("frozen", [False, True])
def test_scripted_and_frozen_agents(frozen):
    """WS-8 among static / non-cooperative / ORCA agents (the ORCA instantiation); with frozen-network agents and a second weight-sharing
    network for them (the frozen instantiation: a second row-list pass)"""
    over = dict(MIX, gen_frozen_fraction=0.3) if frozen else dict(MIX)
    for net in NETS:
        ref, ref_state, log = _reference(64, 4, 7, net, frozen=frozen, **over)
        assert _report(64, 4, 7, net, ref, log).unique().numel() >= 3
        for spl in SPLS:
            got, got_state = _fused(64, 4, 7, net, spl, frozen=frozen, **over)
            _assert_same(ref, ref_state, got, got_state, (frozen, net, spl), log)
    if frozen:               # the scripted agents really were of every kind, frozen-network ones among them
        from rl_collision_avoidance_amd import _lib
        pol = (ref_state[2] >> _lib.F_POLICY_SHIFT) & _lib.F_POLICY_MASK
        present = (ref_state[2] & _lib.F_PRESENT) != 0
        assert set(pol[present].tolist()) >= {_lib.POLICY_EXTERNAL, _lib.POLICY_FROZEN_NET}


def test_sampled_evaluation():
    """greedy=False: the Philox draw of (seed, row, step counter + t) -- the same numbers as the step-by-step path draws"""
    for net in ("straight", "free"):
        ref, ref_state, log = _reference(64, 4, 7, net, greedy=False)
        got, got_state = _fused(64, 4, 7, net, 7, greedy=False)
        _assert_same(ref, ref_state, got, got_state, ("sampled", net), log)
    # (and the draw matters: the sampled round is not the greedy one)
    greedy = _reference(64, 4, 7, "free")[0]
    assert not torch.equal(greedy["per_agent"]["ret"], ref["per_agent"]["ret"]) or greedy["env_steps"] != ref["env_steps"]


def test_many_tiles_two_workgroups_per_cu():
    """4 x 8192: 512 tiles, two workgroups per CU -- one tile's env step under another's matrix phase"""
    ref, ref_state, log = _reference(8192, 4, 7, "straight")
    _report(8192, 4, 7, "straight", ref, log)
    got, got_state = _fused(8192, 4, 7, "straight", 16)
    _assert_same(ref, ref_state, got, got_state, "4 x 8192", log)


def _raw(env, pol, rec, n, frozen=None, buffers=None, fn="cavoid_eval_run_ws"):
    return tw.raw(fn, env, pol, rec, n, frozen, buffers=buffers)


def test_launch_edges_at_the_raw_entry_point():
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords
    W, N, M = 64, 4, 7
    env = _env(W, N, M, 21)
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
    narrow = _policy(_cfg(N, 3), "free")                       # handles that do not describe the same batch: a policy of another width
    assert _raw(env, narrow, rec, 4) == EINVAL
    assert _raw(env, pol, rec, -1) == EINVAL
    # what the kernel does not carry
    rnn = _policy(env.config, "free", arch="rnn")
    ring = _policy(_cfg(N, 24), "free", ws_crowd=True)
    assert _raw(env, rnn, rec, 4) == EUNSUPPORTED            # an rnn handle (cavoid_eval_run's)
    assert _raw(env, ring, rec, 4) == EUNSUPPORTED           # a ws_crowd handle: the ring form
    assert _raw(env, pol, rec, 4, frozen=rnn) == EUNSUPPORTED          # an rnn frozen handle beside a weight-sharing learner
    assert _raw(env, pol, rec, 4, frozen=ring) == EUNSUPPORTED
    assert _raw(env, pol, rec, 4, frozen=narrow) == EUNSUPPORTED       # a weight-sharing frozen handle of another shape
    assert _raw(env, pol, rec, 4, fn="cavoid_eval_run") == EUNSUPPORTED          # ... and cavoid_eval_run still refuses the weight-sharing handle
    assert _raw(env, pol, rec, 0, fn="cavoid_eval_run") == EUNSUPPORTED
    mixed = _env(W, N, M, 21, **dict(MIX, gen_frozen_fraction=0.3))    # frozen-network agents without their network
    mixed.reset()
    mrec = _EvalRecords(mixed)
    assert _raw(mixed, pol, mrec, 4) == EUNSUPPORTED
    mixed.close()
    assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    rnn.close(); ring.close(); narrow.close()
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
    ref, _, log = _reference(W, N, M, "straight")
    assert torch.equal(rec.world_steps, log.world_steps().to(rec.world_steps.device))
    assert torch.equal(rec.ret, log.masked_return(N)[0])
    pol.close(); env.close()


def test_fused_ws_is_refused_with_its_reason_where_it_does_not_apply():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate, evaluate_fused_unavailable_reason, evaluate_fused_ws_unavailable_reason
    env = _env(64, 4, 7, 21, **dict(MIX, gen_frozen_fraction=0.3))
    pol = _policy(env.config, "free")
    rnn = _policy(env.config, "free", arch="rnn")
    assert "frozen" in evaluate_fused_ws_unavailable_reason(env, pol, None)
    assert "frozen policy" in evaluate_fused_ws_unavailable_reason(env, pol, rnn)
    assert "rnn" in evaluate_fused_ws_unavailable_reason(env, rnn, None)
    assert "weight_sharing" in evaluate_fused_unavailable_reason(env, pol, pol)   # (fused=True keeps naming the network)
    with pytest.raises(ValueError, match="frozen"):
        evaluate(env, pol, fused_ws=True)
    with pytest.raises(ValueError, match="weight_sharing"):
        evaluate(env, pol, frozen_policy=pol, fused=True)
    with pytest.raises(ValueError, match="exclude each other"):
        evaluate(env, pol, frozen_policy=pol, fused=True, fused_ws=True)
    pol.close(); rnn.close(); env.close()


CLI = ["--worlds", "64", "--arch", "weight_sharing", "--observed", "7", "--steps-per-graph", "4"]


def test_train_cli_runs_the_kernel_and_prints_the_same_result():
    fused, plain = tw.cli(CLI + ["--fused-ws-evaluate"]), tw.cli(CLI)
    assert "[Evaluate] fused weight_sharing evaluation kernel (cavoid_eval_run_ws), 4 env steps per launch" in fused
    assert "cavoid_eval_run" not in plain
    last = tw.last_evaluate_line
    assert len(last(fused)) == 1 and last(fused) == last(plain)
    tw.report_cache(FAMILY)      # (a whole run of this file: 6 shapes x 3 networks, 16 x 32 x 2, the two mixes x 3, two sampled rounds, 4 x 8192: 29)
