"""tests/rollout_scripts.py on the CPU: the scripted timelines of tests/test_gpu_rollout_limits.py reach every flush kind (a
condition on the inputs), and the checker that holds the device's store to the oracle rejects what a subtly wrong store returns."""
import numpy as np
import pytest

from tests import rollout_scripts as rs

CASE_IDS = [rs.case_id(c) for c in rs.CASES]


@pytest.mark.parametrize("case", rs.CASES, ids=CASE_IDS)
def test_scripts_reach_every_flush_kind(case):
    tl = rs.case_timeline(case)
    assert tl.prev_obs.shape == (tl.T, case.W, case.N, 1 + case.D) and tl.T >= 2 * (2 * case.time_max + 12)
    n = rs.census(rs.case_expected(case), case.time_max)
    print(rs.case_id(case), n)
    for kind in rs.KINDS:
        if kind == "over_32" and case.time_max < 32:
            assert n[kind] == 0                       # needs more than 32 pending entries
        else:
            assert n[kind] >= 3, (kind, n)
    # worlds with one present agent, worlds with no learner beside agent 0, finished and unfinished episodes
    eps = [e for per_world in tl.episodes for e in per_world]
    assert sum(1 for e in eps if e[2] == 1) >= 3
    assert sum(1 for e in eps if e[2] > 1 and e[3].sum() == 1) >= 3
    exp = rs.case_expected(case)
    assert len(exp.episodes) >= case.W and len(exp.key) > 0


@pytest.mark.parametrize("case", rs.CASES, ids=CASE_IDS)
def test_checker_accepts_the_oracle_and_rejects_the_wrong_flush_length(case):
    tl, exp = rs.case_timeline(case), rs.case_expected(case)
    stats = rs.check(exp, rs.as_rows(exp), rs.as_episode_records(exp))
    assert stats == {"rows": len(exp.key), "returns_differ": 0, "episodes": len(exp.episodes)}
    wrong = rs.expected(tl, case.discount, bool(case.reflush), mutant="tmax_plus_1")
    with pytest.raises(AssertionError):
        rs.check(exp, rs.as_rows(wrong))


@pytest.mark.parametrize("case", [c for c in rs.CASES if c.N == 3 and c.W == 97], ids=lambda c: rs.case_id(c))
def test_checker_rejects_wrong_rules_and_wrong_rows(case):
    tl, exp = rs.case_timeline(case), rs.case_expected(case)
    good = rs.as_rows(exp)
    # a full buffer treated as plain done: the leftover row's return is discounted into the chunk (emitted rows are the same)
    wrong = rs.expected(tl, case.discount, bool(case.reflush), mutant="no_leftover")
    if case.discount > 0.0:                           # (discount 0: every return is the raw reward under either rule)
        with pytest.raises(AssertionError, match="return off"):
            rs.check(exp, rs.as_rows(wrong))
        wrong = rs.expected(tl, case.discount, bool(case.reflush), mutant="bootstrap_on_done")
        with pytest.raises(AssertionError, match="return off"):
            rs.check(exp, rs.as_rows(wrong))
    mid = len(exp.key) // 2
    drop = np.arange(len(exp.key)) != mid
    with pytest.raises(AssertionError, match="missing"):
        rs.check(exp, rs.Rows(good.x[drop], good.r[drop], good.a[drop], good.src[drop]))
    twice = np.append(np.arange(len(exp.key)), mid)
    with pytest.raises(AssertionError, match="twice"):
        rs.check(exp, rs.Rows(good.x[twice], good.r[twice], good.a[twice], good.src[twice]))
    moved = good.r.copy()
    moved[mid] = np.float32(moved[mid] + 2 * np.spacing(np.abs(moved[mid])))
    with pytest.raises(AssertionError, match="return off"):
        rs.check(exp, rs.Rows(good.x, moved, good.a, good.src))
    one = good.r.copy()                               # one spacing is the bound itself: accepted, and counted
    one[mid] = np.nextafter(one[mid], np.float32(np.inf))
    assert rs.check(exp, rs.Rows(good.x, one, good.a, good.src))["returns_differ"] == 1
    # x by one bit, an action, an episode's length, a missing episode record
    bent = good.x.copy()
    bent[mid, 0] = np.nextafter(bent[mid, 0], np.float32(np.inf))
    with pytest.raises(AssertionError, match="x differs"):
        rs.check(exp, rs.Rows(bent, good.r, good.a, good.src))
    acts = good.a.copy()
    acts[mid] = (acts[mid] + 1) % 11
    with pytest.raises(AssertionError, match="action differs"):
        rs.check(exp, rs.Rows(good.x, good.r, acts, good.src))
    eps = rs.as_episode_records(exp)
    longer = eps.copy()
    longer[len(eps) // 2, 2] += 1
    with pytest.raises(AssertionError, match="total_length"):
        rs.check(exp, good, longer)
    with pytest.raises(AssertionError, match="episode records"):
        rs.check(exp, good, eps[:-1])


def test_subset_mode_and_duplicate_split():
    """what the capacity tests lean on: ``subset`` lets rows be missing and nothing else; the rings hold first emissions, the append
    buffer the re-emissions"""
    case = rs.Case(2, 1, 0.97, **rs.SMALL)
    exp = rs.case_expected(case)
    main, dup = rs.split_duplicates(exp)
    assert len(main.key) + len(dup.key) == len(exp.key) and len(dup.key) == rs.census(exp, 2)["reflush_dup"]
    first = {}
    for k in exp.key:
        first[tuple(k[:3])] = min(first.get(tuple(k[:3]), 1 << 30), k[3])
    assert all(first[tuple(k[:3])] == k[3] for k in main.key) and all(first[tuple(k[:3])] < k[3] for k in dup.key)
    good, eps = rs.as_rows(dup), rs.as_episode_records(exp)
    some = np.arange(len(dup.key)) % 3 == 0
    assert rs.check(dup, rs.Rows(*(v[some] for v in good)), subset=True)["rows"] == int(some.sum())
    with pytest.raises(AssertionError, match="missing"):
        rs.check(dup, rs.Rows(*(v[some] for v in good)))
    twice = np.array([0, 3, 3])
    with pytest.raises(AssertionError, match="twice"):
        rs.check(dup, rs.Rows(*(v[twice] for v in good)), subset=True)
    with pytest.raises(AssertionError, match="unexpected"):
        rs.check(dup, rs.Rows(*(v[:5] for v in rs.as_rows(main))), subset=True)
    assert rs.check(exp, rs.as_rows(exp), eps[::2], subset=True)["episodes"] == len(eps[::2])
    with pytest.raises(AssertionError):
        rs.check(exp, rs.as_rows(exp), np.concatenate([eps[:1], eps[:1]]), subset=True)      # the same record twice


def test_deep_flush_counts():
    # world 0 agent 1: a chunk of 33 rows emitted at step 40 (recorded 7 .. 39), then one of 2 rows; world 1: 31 rows emitted at 31
    src = [(0, 1, t, 40) for t in range(7, 40)] + [(0, 1, 40, 42), (0, 1, 41, 42)] + [(1, 0, t, 31) for t in range(0, 31)]
    assert rs.deep_flush_counts(np.array(src), 33) == (1, 2)         # reaches 33 and 32
    assert rs.deep_flush_counts(np.array(src), 31) == (1, 4)         # 31 or more: those two, 9 -> 40 and 0 -> 31
