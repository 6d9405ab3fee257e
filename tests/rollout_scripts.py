"""Scripted input for the experience store (csrc/cavoid_rollout.hpp) at the limits of what its C ABI accepts, the census that
says which flush branches a script reaches, and the checker that holds a drained store to oracle/rollout_oracle.py.

Pure numpy, no GPU and no reference: tests/test_rollout_scripts.py runs the conditions on the inputs and the checker's rejection
cases on the CPU, tests/test_gpu_rollout_limits.py feeds the same timelines to ``cavoid_rollout_push``.

A TIMELINE is, per world, a run of back-to-back scripted episodes cut at a common step count (the last one is usually unfinished).
An episode fixes who is present, who learns, per-step rewards, monotone done flags, actions and values; the model is
``make_script`` of tests/golden/make_rollout_golden.py (not imported: the maker puts the reference on ``sys.path``).  What chance
does not give is forced, one kind per episode in turn (``FORCED``)."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from oracle import rollout_oracle as ro

KINDS = ("single", "leftover", "done_short", "time_max", "reflush_dup", "over_32")
FORCED = ("first", "full", "double", "early", "alone", "solo_learner", "free")

Timeline = namedtuple("Timeline", "time_max W N D T prev_obs actions values rewards done game_over episodes")
#   prev_obs f32 [T, W, N, 1+D] (column 0 = is_learning), actions i32 / values f32 / rewards f32 / done u8 [T, W, N],
#   game_over u8 [T, W] ("every present learning agent done"), episodes: per world [(start, stop, n_present, learning[N])]
Expected = namedtuple("Expected", "chunks key x r a episodes")
#   chunks: [(world, episode start, oracle Chunk)] as the oracle yielded them (before the cleaned mode's filter: the census reads these)
#   key i64 [n, 4] (world, agent, recorded-at, emitted-at), x f32 [n, D], r f64 [n], a i64 [n]: the rows a drain must return
#   episodes: [(world, total_reward f64, total_length)] of the FINISHED episodes, per world in time order
Rows = namedtuple("Rows", "x r a src")
#   what a drain returns: x f32 [n, D], r f32 [n], a int [n], src int [n, 4]


def make_episode(rng, N, D, time_max, max_len, force):
    """One scripted episode (after ``make_script``): returns (T, n_present, learning, finish)."""
    n_present = int(rng.integers(1, N + 1))
    learning = np.zeros(N, bool)
    finish = rng.integers(1, max_len + 1, size=N)
    if force in ("first", "early"):
        n_present = max(n_present, 2)
    elif force == "alone":
        n_present = 1
    elif force == "solo_learner":
        n_present = N
    learning[:n_present] = rng.random(n_present) < 0.75
    learning[0] = True
    if force == "first":                 # done at its first step: a one-entry buffer flushes; the world goes on (re-flush quirk)
        for i in range(1, min(n_present, 3)):
            learning[i], finish[i] = True, 1
        finish[0] = max(finish[0], time_max + 3)
    elif force == "full":                # done with exactly time_max + 1 pending: the leftover chunk
        finish[0] = time_max + 1
    elif force == "double":              # the same after one time-max flush
        finish[0] = 2 * time_max + 1
    elif force == "early":               # done long before its world ends: the re-flush quirk's duplicates
        learning[1], finish[1], finish[0] = True, 2, max_len
    elif force == "solo_learner":
        learning[1:] = False
    T = int(finish[:n_present][learning[:n_present]].max())
    return T, n_present, learning, finish


@functools.lru_cache(maxsize=None)
def timeline(time_max, W, N, D, seed=0, episodes=2.5):
    """The scripted timeline of one shape: a pure function of its arguments.  Episodes run up to ``2 * time_max + 12`` steps and the
    timeline is cut after ``episodes`` times that."""
    rng = np.random.default_rng([seed, time_max, W, N, D])
    max_len = 2 * time_max + 12
    T = int(episodes * max_len)
    learn = np.zeros((T, W, N), bool)
    present = np.zeros((T, W, N), bool)
    done = np.zeros((T, W, N), np.uint8)
    game_over = np.zeros((T, W), np.uint8)
    eps = []
    for w in range(W):
        start, e, mine = 0, 0, []
        while start < T:
            Te, n_present, learning, finish = make_episode(rng, N, D, time_max, max_len, FORCED[(w + e) % len(FORCED)])
            stop = min(start + Te, T)
            learn[start:stop, w] = learning
            present[start:stop, w, :n_present] = True
            for i in range(n_present):
                if finish[i] <= Te:
                    done[start + finish[i] - 1:stop, w, i] = 1
            if start + Te <= T:
                game_over[start + Te - 1, w] = 1
            mine.append((start, stop, n_present, learning))
            start, e = stop, e + 1
        eps.append(mine)
    prev_obs = np.round(rng.normal(0, 1, size=(T, W, N, 1 + D)), 1).astype(np.float32)        # coarse floats
    prev_obs[..., 0] = learn
    prev_obs[~present] = 0.0
    actions = rng.integers(0, 11, size=(T, W, N)).astype(np.int32)
    values = np.round(rng.normal(0, 0.5, size=(T, W, N)), 3).astype(np.float32)
    rewards = np.round(rng.normal(0, 0.2, size=(T, W, N)), 3).astype(np.float32)
    # "every present learning agent done", restated from the arrays the store sees
    pl = present & learn
    assert np.array_equal(game_over.astype(bool), np.all(done.astype(bool) | ~pl, axis=2) & pl.any(axis=2))
    return Timeline(time_max, W, N, D, T, prev_obs, actions, values, rewards, done, game_over, eps)


def _oracle_chunks(tl, w, start, stop, n_present, learning, gamma, t_max):
    sl = slice(start, stop)
    obs = tl.prev_obs[sl, w].astype(np.float64)
    obs = np.concatenate([obs, obs[-1:]])                                  # (the oracle never reads the last entry)
    return ro.run_episode(obs, tl.rewards[sl, w].astype(np.float64), tl.done[sl, w].astype(bool), learning, n_present,
                          tl.actions[sl, w], tl.values[sl, w].astype(np.float64), gamma, t_max)


def _drop_reflushes(chunks, done):
    """cleaned mode (reflush_done = 0): what a done-and-trained agent would re-flush is not recorded"""
    trained_at, kept = {}, []
    for c in chunks:
        if c.agent in trained_at and c.emitted_t > trained_at[c.agent]:
            continue
        kept.append(c)
        if done[c.emitted_t, c.agent]:
            trained_at.setdefault(c.agent, c.emitted_t)
    return kept


MUTANTS = ("tmax_plus_1", "no_leftover", "bootstrap_on_done")


def expected(tl, gamma, reflush=True, mutant=None):
    """Every row and every episode record the store owes for ``tl``, from the oracle.  ``mutant`` names a deliberately WRONG rule
    (the rejection cases of the checker): the flush rule at ``t_max + 1``, a full buffer treated as plain done, a bootstrap value
    applied on done."""
    t_max = tl.time_max + (1 if mutant == "tmax_plus_1" else 0)
    real = ro.n_step_returns
    if mutant == "no_leftover":
        ro.n_step_returns = lambda buf, g, boot, done, tm: real(buf, g, boot, done, 1 << 30)
    elif mutant == "bootstrap_on_done":
        ro.n_step_returns = lambda buf, g, boot, done, tm: real(buf, g, 0.5 if done else boot, done, tm)
    else:
        assert mutant in (None, "tmax_plus_1"), mutant
    try:
        chunks, keys, xs, rs, as_, episodes = [], [], [], [], [], []
        for w in range(tl.W):
            for start, stop, n_present, learning in tl.episodes[w]:
                cs = _oracle_chunks(tl, w, start, stop, n_present, learning, gamma, t_max)
                chunks += [(w, start, c) for c in cs]
                if not reflush:
                    cs = _drop_reflushes(cs, tl.done[start:stop, w])
                for c in cs:
                    for row, t in enumerate(c.t):
                        keys.append((w, c.agent, start + t, start + c.emitted_t))
                    xs.append(c.x.reshape(len(c.r), -1)); rs.append(c.r); as_.append(np.argmax(c.a, axis=1))
                if tl.game_over[stop - 1, w]:
                    # run(): total_reward += reward_sum, total_length += len(r_) + 1 per yield (ProcessAgent.py:236-237)
                    episodes.append((w, float(sum(c.score for c in cs)), int(sum(len(c.r) + 1 for c in cs))))
    finally:
        ro.n_step_returns = real
    x = np.concatenate(xs)
    x32 = x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x)                       # the scripts' observations are float32 values
    return Expected(chunks, np.array(keys, dtype=np.int64).reshape(-1, 4), x32, np.concatenate(rs), np.concatenate(as_).astype(np.int64),
                    episodes)


def as_rows(exp):
    """the drain a correct store would return for ``exp`` (returns cast to float32 like the device's store)"""
    return Rows(exp.x.copy(), exp.r.astype(np.float32), exp.a.copy(), exp.key.copy())


def as_episode_records(exp):
    return np.array([(w, np.float32(tr), tl) for w, tr, tl in exp.episodes], dtype=np.float32).reshape(-1, 3)


def census(exp, time_max):
    """The six flush kinds of the oracle's chunks (the reference side, whatever ``reflush`` the rows were built with):
      single       flushes of a one-entry buffer (an agent done at the first step of its chunk)
      leftover     the separate one-row chunk of "done with a full buffer"
      done_short   first done flushes of 2 .. time_max entries (time_max = 1 leaves no such length: there, of one entry)
      time_max     flushes by the step count: time_max rows, the newest entry kept back
      reflush_dup  rows emitted a second time: a done-and-trained agent's kept seed
      over_32      flushes with more than 32 pending entries (the device's register form holds 32)"""
    n = dict.fromkeys(KINDS, 0)
    seen = {}
    for w, start, c in exp.chunks:
        emitted = seen.setdefault((w, start, c.agent), set())
        if c.leftover:
            n["leftover"] += 1
        else:
            pending = c.emitted_t - c.t[0] + 1
            with_newest = c.t[-1] == c.emitted_t
            again = c.t[0] in emitted
            n["reflush_dup"] += sum(1 for t in c.t if t in emitted)
            n["single"] += pending == 1
            n["done_short"] += with_newest and not again and min(2, time_max) <= pending <= time_max
            n["time_max"] += (not with_newest) and len(c.t) == time_max
            n["over_32"] += pending > 32
        emitted.update(c.t)
    return n


def _pack(key):
    key = np.asarray(key).astype(np.int64).reshape(-1, 4)
    assert key.min(initial=0) >= 0 and key[:, 1].max(initial=0) < 256 and key[:, 2:].max(initial=0) < 1 << 20, "provenance out of range"
    return (key[:, 0] << 48) | (key[:, 1] << 40) | (key[:, 2] << 20) | key[:, 3]


def _unpack(v):
    return (int(v >> 48), int(v >> 40) & 255, int(v >> 20) & 0xFFFFF, int(v) & 0xFFFFF)


def split_duplicates(exp):
    """(main, dup): the rows that live in the (step, slot) rings -- the first emission of every recorded experience -- and the
    re-flush quirk's re-emissions, which the store appends to its duplicate buffer.  Episode records stay with ``main``."""
    packed = _pack(exp.key)
    order = np.argsort(packed, kind="stable")                              # (world, agent, recorded-at), then emitted-at
    first = np.ones(len(packed), bool)
    same = (packed[order][1:] >> 20) == (packed[order][:-1] >> 20)
    first[order[1:][same]] = False
    part = lambda m, eps: Expected(exp.chunks, exp.key[m], exp.x[m], exp.r[m], exp.a[m], eps)
    return part(first, exp.episodes), part(~first, [])


def check(expected_chunks, rows, episodes=None, subset=False):
    """Hold what a drain returned (``rows``: x, r, a, src; ``episodes`` [k, 3] or None) to ``expected_chunks``.  Raises
    AssertionError; returns {"rows", "returns_differ", "episodes"} -- ``returns_differ`` counts the returns that are not
    ``np.float32(oracle r)`` bit for bit.

    x bit-equal, action equal, (world, agent, recorded-at, emitted-at) matched one to one -- nothing missing, nothing extra, nothing
    twice.  (The oracle replays the unfinished last episode of a world too, so rows of unfinished episodes are expected like any
    other.)  ``subset=True`` (a store that ran out of capacity) lets rows be missing, nothing else.
    The return within ONE float32 spacing of np.float32(oracle r): the device runs the same float64 recurrence, an fma contraction
    moves it by at most a double ulp per term, so the float32 cast can differ only at a rounding boundary.  Episode records: world
    and total_length exact, total_reward within one float32 spacing (the double sums differ only in the order of the atomics);
    with ``subset`` they are distinct members of the expected records."""
    exp = expected_chunks
    x, r, a, src = (np.asarray(v) for v in rows)
    assert x.dtype == np.float32 and r.dtype == np.float32 and x.shape == (len(r), exp.x.shape[1]) and len(a) == len(r) == len(src)
    got_keys, want_keys = _pack(src), _pack(exp.key)
    eo = np.argsort(want_keys)
    want_sorted = want_keys[eo]
    assert len(want_sorted) < 2 or (want_sorted[1:] != want_sorted[:-1]).all(), "the oracle's keys are not unique"
    missing, extra = np.setdiff1d(want_keys, got_keys), np.setdiff1d(got_keys, want_keys)
    assert subset or missing.size == 0, "%d rows missing, first (world, agent, recorded, emitted) = %r" % (missing.size, _unpack(missing[0]))
    assert extra.size == 0, "%d rows unexpected, first %r" % (extra.size, _unpack(extra[0]))
    assert len(np.unique(got_keys)) == len(got_keys), "%d rows, %d distinct: a row came twice" % (len(got_keys), len(np.unique(got_keys)))
    at = eo[np.searchsorted(want_sorted, got_keys)]                        # the expected row of every returned row
    assert np.array_equal(want_keys[at], got_keys)
    bad = np.flatnonzero((x.view(np.uint32) != exp.x[at].view(np.uint32)).any(axis=1))
    assert bad.size == 0, "x differs in %d rows, first %r" % (bad.size, _unpack(got_keys[bad[0]]))
    bad = np.flatnonzero(a.astype(np.int64) != exp.a[at])
    assert bad.size == 0, "action differs in %d rows, first %r" % (bad.size, _unpack(got_keys[bad[0]]))
    want = exp.r[at].astype(np.float32)
    err = np.abs(r.astype(np.float64) - want.astype(np.float64))
    bad = np.flatnonzero(~(err <= np.spacing(np.abs(want)).astype(np.float64)))
    assert bad.size == 0, "return off by more than one float32 spacing in %d rows, first %r: %r for %r" % (
        bad.size, _unpack(got_keys[bad[0]]), r[bad[0]], exp.r[at][bad[0]])
    stats = {"rows": int(len(r)), "returns_differ": int(np.count_nonzero(r != want)), "episodes": 0}
    if episodes is not None:
        ep = np.asarray(episodes, dtype=np.float32).reshape(-1, 3)
        assert subset or len(ep) == len(exp.episodes), "%d episode records for %d finished episodes" % (len(ep), len(exp.episodes))
        per_world = {}
        for w, total_reward, total_length in exp.episodes:                 # a world's records arrive in time order
            per_world.setdefault(w, []).append((total_reward, total_length))
        for rec in ep:
            w = int(rec[0])
            assert rec[0] == w and per_world.get(w), "a record of world %r that finished no (further) episode" % (rec[0],)
            near = lambda e: abs(float(rec[1]) - float(np.float32(e[0]))) <= float(np.spacing(np.abs(np.float32(e[0]))))
            if subset:                                                     # any not yet matched episode of that world
                hit = [k for k, e in enumerate(per_world[w]) if e[1] == rec[2] and near(e)]
                assert hit, ("no finished episode matches the record", tuple(rec), per_world[w])
                per_world[w].pop(hit[0])
                continue
            total_reward, total_length = e = per_world[w].pop(0)
            assert rec[2] == total_length, ("total_length", w, rec[2], total_length)
            assert near(e), ("total_reward", w, rec[1], total_reward)
        stats["episodes"] = len(ep)
    return stats


# ---- the cases of tests/test_gpu_rollout_limits.py (the host test holds the census condition for each) -----------------------
Case = namedtuple("Case", "time_max reflush discount W N D")
SMALL = dict(W=97, N=3, D=6)          # 291 slots: two 256-thread blocks, a ragged last wavefront
CASES = tuple(Case(tm, rf, 0.97, **SMALL) for tm in (1, 2, 31, 32, 33, 40) for rf in (1, 0)) + (
    Case(33, 1, 1.0, **SMALL), Case(33, 1, 0.0, **SMALL),
    Case(254, 1, 0.97, W=22, N=3, D=6),
    Case(33, 1, 0.97, W=13, N=20, D=453))      # worlds straddle wavefront and block edges, the widest row the env makes


def case_id(c):
    return "tmax%d-reflush%d-g%g-W%dN%dD%d" % c


def case_timeline(c):
    return timeline(c.time_max, c.W, c.N, c.D)


@functools.lru_cache(maxsize=None)
def case_expected(c):
    """computed once per case and shared: treat as read-only"""
    return expected(case_timeline(c), c.discount, bool(c.reflush))


# ---- the fused forms' equality tests on the real env (tests/test_gpu_actor.py and its neighbours) ------------------------------
DEEP_BAR = 20


def deep_flush_counts(src, time_max):
    """From a drain's provenance [n, 4]: (chunks of exactly ``time_max`` rows -- a flush by the step count --, emissions that reach
    back ``min(time_max, 32)`` steps or more: past the 32 registers of the device's backward pass where time_max allows it, its
    last register at time_max = 31)."""
    src = np.asarray(src).astype(np.int64).reshape(-1, 4)
    chunk = (src[:, 0] << 40) | (src[:, 1] << 32) | src[:, 3]
    _, rows = np.unique(chunk, return_counts=True)
    return int(np.count_nonzero(rows == time_max)), int(np.count_nonzero(src[:, 3] - src[:, 2] >= min(time_max, 32)))


def require_deep_flushes(src, time_max, what):
    """a condition on a case's INPUTS (not a measurement): the step-by-step side took the long backward pass often enough"""
    chunks, far = deep_flush_counts(src, time_max)
    print("%s: time_max %d: %d chunks of exactly time_max rows, %d emissions reaching back %d steps or more"
          % (what, time_max, chunks, far, min(time_max, 32)))
    assert chunks >= DEEP_BAR and far >= DEEP_BAR, (what, time_max, chunks, far)
