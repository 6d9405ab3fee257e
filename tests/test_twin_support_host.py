"""CPU tests of the comparison helpers every twin test goes through (tests/actor_twins.py, tests/eval_twins.py): they are the single place
where a field could drop out of every form's test at once.  Stand-ins made of small CPU tensors -- 2 worlds x 3 agents, a ring of 4 --
compare equal, and one changed element of any field, on one side, raises AssertionError with that field's name in its message."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import actor_twins as at
from tests import eval_twins as et

W, N, RING, TOTAL = 2, 3, 4, 7
ENV_TENSORS = ("state f64", "state f32", "state flags", "episode", "rewards", "done", "game_over")
ROLL_TENSORS = ("obs", "x", "val", "ret", "act_ring", "emit_t", "dup_count")


def _twin():
    """(env, rollout) stand-ins; every tensor is filled with distinct values"""
    g = torch.Generator().manual_seed(5)
    f = lambda *shape: torch.rand(shape, generator=g)
    i = lambda *shape: torch.randint(0, 9, shape, generator=g, dtype=torch.int32)
    state = [f(5, W * N).double(), f(4, W * N), i(W * N)]
    env = SimpleNamespace(get_state=lambda: state, episode=i(W), rewards=f(W, N), done=i(W, N).to(torch.uint8), game_over=i(W).to(torch.uint8))
    roll = SimpleNamespace(obs=f(W, N, 11), x=f(RING, W * N, 10), val=f(RING, W * N), ret=f(RING, W * N), act_ring=i(RING, W * N),
                           emit_t=i(RING, W * N), dup_count=i(2), step_index=TOTAL)
    return env, roll


def _tensor(env, roll, name):
    if name.startswith("state "):
        return env.get_state()[at.STATE.index(name)]
    return getattr(env if name in ENV_TENSORS else roll, name)


def _bump(t):
    """one element changed, in place"""
    flat = t.view(-1)
    flat[flat.numel() // 2] = flat[flat.numel() // 2] + 1


def test_compare_twins_passes_on_equal_twins():
    (env_a, a), (env_b, b) = _twin(), _twin()
    at.compare_twins(env_a, a, env_b, b, TOTAL, case="equal")
    at.compare_interleaved(env_a, a, env_b, b, case="equal")


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("name", ENV_TENSORS + ROLL_TENSORS)
def test_compare_twins_names_the_field_that_differs(name, side):
    (env_a, a), (env_b, b) = _twin(), _twin()
    _bump(_tensor(env_a, a, name) if side == "a" else _tensor(env_b, b, name))
    with pytest.raises(AssertionError) as err:
        at.compare_twins(env_a, a, env_b, b, TOTAL, case="one element")
    assert name in str(err.value) and str(TOTAL) in str(err.value) and "one element" in str(err.value)


def test_compare_twins_holds_the_step_counter_on_both_sides_and_to_the_total():
    for who, index, total in (("a", TOTAL + 1, TOTAL), ("b", TOTAL + 1, TOTAL), (None, TOTAL, TOTAL + 1)):
        (env_a, a), (env_b, b) = _twin(), _twin()
        if who is not None:
            (a if who == "a" else b).step_index = index
        with pytest.raises(AssertionError) as err:
            at.compare_twins(env_a, a, env_b, b, total)
        assert "step_index" in str(err.value)


def test_compare_twins_without_dup_count_is_the_tile_forms_choice_by_argument():
    """the default compares dup_count; only a call that names the narrower set leaves it out"""
    (env_a, a), (env_b, b) = _twin(), _twin()
    _bump(a.dup_count)
    at.compare_twins(env_a, a, env_b, b, TOTAL, rings=at.RINGS)
    with pytest.raises(AssertionError) as err:
        at.compare_twins(env_a, a, env_b, b, TOTAL)
    assert "dup_count" in str(err.value)


@pytest.mark.parametrize("name", ("obs",) + at.STATE + at.RINGS)
def test_compare_interleaved_names_the_field_that_differs(name):
    (env_a, a), (env_b, b) = _twin(), _twin()
    _bump(_tensor(env_b, b, name))
    with pytest.raises(AssertionError) as err:
        at.compare_interleaved(env_a, a, env_b, b, case="turns")
    assert name in str(err.value) and "interleaved" in str(err.value)
    if name not in at.INTERLEAVE_TILE:                       # the tile forms' narrower set does not look at it: an argument, not the default
        at.compare_interleaved(env_a, a, env_b, b, at.INTERLEAVE_TILE)


def _batch(order):
    """a drained batch of 6 rows in the given order; src = (world, agent, step) is what the rows are sorted by"""
    g = torch.Generator().manual_seed(9)
    src = torch.tensor([[w, n, 3] for w in range(W) for n in range(N)], dtype=torch.int32)
    rows = SimpleNamespace(src=src, x=torch.rand((6, 10), generator=g), r=torch.rand(6, generator=g),
                           a_index=torch.randint(0, 11, (6,), generator=g))
    order = torch.tensor(order)
    return SimpleNamespace(**{k: getattr(rows, k)[order].clone() for k in at.DRAINED})


def test_compare_drained_sorts_by_provenance_and_names_the_field_that_differs():
    at.compare_drained(_batch([0, 1, 2, 3, 4, 5]), _batch([5, 3, 1, 0, 2, 4]), "two arrival orders")
    for name in at.DRAINED:
        ba, bb = _batch([0, 1, 2, 3, 4, 5]), _batch([5, 3, 1, 0, 2, 4])
        _bump(getattr(bb, name))
        with pytest.raises(AssertionError) as err:
            at.compare_drained(ba, bb, "one element")
        assert name in str(err.value) and "drained" in str(err.value)


def test_compare_episode_records_exact_counters_and_totals_to_float32_rounding():
    ea = np.array([[3.0, 1.25, 40.0], [1.0, -0.5, 12.0], [2.0, 0.75, 33.0]])
    at.compare_episode_records(ea, ea[[2, 0, 1]].copy(), "two arrival orders")
    near = ea.copy()
    near[:, 1] += 5e-7                                       # inside rtol = atol = 1e-6: the order of the double atomics
    at.compare_episode_records(ea, near, "float32 rounding")
    far = ea.copy()
    far[1, 1] += 1e-5
    with pytest.raises(AssertionError) as err:
        at.compare_episode_records(ea, far, "a total")
    assert "column 1" in str(err.value)
    for col in (0, 2):
        off = ea.copy()
        off[1, col] += 5e-7                                  # the counters are exact: no tolerance
        with pytest.raises(AssertionError) as err:
            at.compare_episode_records(ea, off, "a counter")
        assert "column %d" % col in str(err.value)


# ---- eval_twins._assert_same -----------------------------------------------------------------------------------------------------------
def _result():
    """(result dict, world buffer) of a round of 2 worlds x 3 agents, hand-made"""
    per = {"learning": torch.tensor([True, True, False, True, True, True]), "outcome": torch.tensor([1, 2, 0, 3, 1, 1], dtype=torch.int32),
           "ret": torch.tensor([0.5, -0.25, 0.0, 1.0, 0.125, -1.0], dtype=torch.float64)}
    res = {"agents": 5, "env_steps": 3, "success_rate": 0.6, "mean_reward": float(per["ret"][per["learning"]].sum()) / 5, "per_agent": per}
    state = [torch.arange(12, dtype=torch.float64).view(2, 6), torch.arange(6, dtype=torch.float32).view(1, 6), torch.arange(6, dtype=torch.int32)]
    return res, state


def test_assert_same_passes_on_equal_results():
    (ref, ref_state), (got, got_state) = _result(), _result()
    et._assert_same(ref, ref_state, got, got_state, "equal")


def _fails(ref, ref_state, got, got_state, word, **kw):
    with pytest.raises(AssertionError) as err:
        et._assert_same(ref, ref_state, got, got_state, "one change", **kw)
    assert word in str(err.value) and "one change" in str(err.value), str(err.value)


def test_assert_same_fails_on_a_scalar_a_key_order_and_a_dtype():
    (ref, ref_state), (got, got_state) = _result(), _result()
    got["success_rate"] = 0.61
    _fails(ref, ref_state, got, got_state, "success_rate")
    got, _ = _result()
    got["env_steps"] = 3.0                                   # equal, but a float where the loop has an int
    _fails(ref, ref_state, got, got_state, "env_steps")
    got, _ = _result()
    got = {k: got[k] for k in ("env_steps", "agents", "success_rate", "mean_reward", "per_agent")}
    _fails(ref, ref_state, got, got_state, "keys")
    got, _ = _result()
    got["per_agent"]["outcome"] = got["per_agent"]["outcome"].to(torch.int64)   # equal values, another dtype
    _fails(ref, ref_state, got, got_state, "outcome")


@pytest.mark.parametrize("name", ["learning", "outcome", "ret"])
def test_assert_same_fails_on_each_per_agent_tensor(name):
    (ref, ref_state), (got, got_state) = _result(), _result()
    t = got["per_agent"][name]
    t[1] = ~t[1] if t.dtype == torch.bool else t[1] + 1
    _fails(ref, ref_state, got, got_state, name)


@pytest.mark.parametrize("index,name", [(0, "f64"), (1, "f32"), (2, "flags")])
def test_assert_same_fails_on_each_state_tensor(index, name):
    (ref, ref_state), (got, got_state) = _result(), _result()
    _bump(got_state[index])
    _fails(ref, ref_state, got, got_state, name)


def _log():
    """2 worlds x 3 agents, 3 steps; world 0 is over at step 2 and its agent 1 is paid -0.25 at step 3, after that"""
    log = et._StepLog.__new__(et._StepLog)
    log.rew = [torch.tensor([0.5, 0.0, 0.0, 0.25, 0.0, 0.0]), torch.tensor([0.0, 1.0, 0.0, 0.25, 0.5, 0.0]),
               torch.tensor([0.0, -0.25, 0.0, 0.5, 0.0, -1.0])]
    log.over = [torch.tensor([0, 0], dtype=torch.uint8), torch.tensor([1, 0], dtype=torch.uint8), torch.tensor([1, 1], dtype=torch.uint8)]
    return log


def _round_with_log():
    """the loop's result (it sums on after a world is over) and the kernel's (the masked definition) of the round _log() describes"""
    log = _log()
    masked, paid_after = log.masked_return(N)
    assert paid_after.tolist() == [False, True, False, False, False, False] and list(log.world_steps()) == [2, 3]
    loop = torch.stack(log.rew).double().sum(0)
    assert loop[1] == 0.75 and masked[1] == 1.0              # the two definitions differ for the agent paid after its world's end, only
    (ref, ref_state), (got, got_state) = _result(), _result()
    learning = ref["per_agent"]["learning"]
    ref["per_agent"]["ret"], got["per_agent"]["ret"] = loop, masked.clone()
    ref["mean_reward"] = float(loop[learning].sum()) / 5
    got["mean_reward"] = float(masked[learning].sum()) / 5
    return log, ref, ref_state, got, got_state


def test_assert_same_holds_the_return_to_its_definition_for_every_agent():
    log, ref, ref_state, got, got_state = _round_with_log()
    et._assert_same(ref, ref_state, got, got_state, "the two definitions", log)
    for agent in range(W * N):                               # the agent paid after its world's end is held to the definition too
        bad = copy.deepcopy(got)
        bad["per_agent"]["ret"][agent] += 0.5
        _fails(ref, ref_state, bad, got_state, "ret against its definition", log=log)
    bad = copy.deepcopy(got)
    bad["mean_reward"] += 0.5
    _fails(ref, ref_state, bad, got_state, "mean_reward", log=log)


def test_assert_same_skips_the_loops_return_only_for_the_agents_paid_after_their_worlds_end():
    log, ref, ref_state, got, got_state = _round_with_log()
    # against the LOOP the paid-after agent is excused ...
    et._assert_same(ref, ref_state, got, got_state, "excused", log)
    # ... and no other: a loop whose sum differs for another agent is a failure (the kernel still meets the definition)
    for agent in (0, 3, 4, 5):
        other = copy.deepcopy(ref)
        other["per_agent"]["ret"][agent] += 0.5
        _fails(other, ref_state, got, got_state, "ret against the loop's", log=log)
    # without a log that says who was paid after the end nothing is skipped: the two definitions' difference fails
    _fails(ref, ref_state, got, got_state, "mean_reward")
    # and where the log says nobody was, mean_reward and ret are compared like every other key
    quiet = _log()
    quiet.rew[2][1] = 0.0
    masked, paid_after = quiet.masked_return(N)
    assert not bool(paid_after.any())
    (ref, ref_state), (got, got_state) = _result(), _result()
    ref["per_agent"]["ret"], got["per_agent"]["ret"] = masked.clone(), masked.clone()
    ref["mean_reward"] = got["mean_reward"] = float(masked[ref["per_agent"]["learning"]].sum()) / 5
    et._assert_same(ref, ref_state, got, got_state, "nobody paid after", quiet)
    got["mean_reward"] += 0.5
    _fails(ref, ref_state, got, got_state, "mean_reward", log=quiet)
