"""CPU side of the tests that take the env step off `cavoid_cfg`'s default numbers (tests/test_gpu_cfg_fields.py, tests/test_gpu_crowd_cfg.py,
the UNCLIPPED + RING case of tests/test_gpu_actor_oracle.py): every case those files run on the GPU is built here from the same table
(tests/cfg_regimes.py) and run through the float64 oracle alone, over the same shape, seed and steps, and held to the conditions that
make it worth running:

  * every field decides something -- the oracle run again with ONE field of the case's set back at its default and the same actions
    leaves the first run (done, game_over, a reward or an observation by more than 1e-5, a flag bit, or the generated state) within the
    case's steps: a form that baked in a default for that field could not pass the case.  The first differing step of every field is
    printed (pytest -s);
  * the events happen -- restarts, collisions, getting-close rewards, both clip ends under CLIPPED, neighbours hidden by the horizon,
    steps paid reward_time_step; goals and time-outs in at least one case per dynamics and form family.

The `topup-` family (tests/test_gpu_topup_oracle.py: the relay launch's ring top-up) is held to conditions of its own: every world reads
records three rings deep, worlds restart at different steps, and what the top-up wavefront loads for itself -- each generator field,
max_time_ratio, world_offset -- decides something in episodes whose records only that wavefront can have made.

These are conditions, not measurements: if a seed or a step count misses one, another is picked in tests/cfg_regimes.py."""
import collections
import functools

import numpy as np
import pytest

from tests import cfg_regimes as R
from tests import replay as rp

TOL = 1e-5
NUMERIC = [c for c in R.CASES if c.fields and c.family != "topup"]
TOPUP = R.select("topup-")


def _state_differs(a, b):
    return (not np.array_equal(a.flags, b.flags)) or (not np.array_equal(a.f32, b.f32)) or float(np.abs(a.f64 - b.f64).max()) > 1e-9


def _step_differs(a, b, sa, sb):
    (oa, ra, da, ga), (ob, rb, db, gb) = a, b
    if not (np.array_equal(da, db) and np.array_equal(ga, gb) and np.array_equal(sa.flags, sb.flags)):
        return True
    return float(np.abs(ra - rb).max()) > TOL or float(rp.obs_diff(oa, ob).max()) > TOL


@functools.lru_cache(maxsize=None)
def _run(cid):
    """(the case's oracle run, {field: first differing step; 0 = the generated state}, the fields that never differed): the base run
    and one run per field in lock-step, a field's run dropped at its first difference"""
    case = R.BY_ID[cid]
    base = R.OracleRun(case)
    live = {f: R.OracleRun(case, **{f: R.field_default(f, case.N)}) for f in case.fields}
    first = {}
    for f in list(live):
        if _state_differs(base.st, live[f].st):
            first[f] = 0
            del live[f]
    for kind, K, n in case.plan:
        _, fed = base.draw(K)
        for t in range(n):
            out = base.step(fed[t])
            for f in list(live):
                if _step_differs(out, live[f].step(fed[t]), base.st, live[f].st):
                    first[f] = base.t
                    del live[f]
    return base, first, sorted(live)


def test_the_sets_leave_every_field_off_its_default_and_the_defaults_are_the_librarys():
    from oracle import c_oracle as co
    for name, fields in list(R.STEP_SETS.items()) + list(R.GEN_SETS.items()):
        for f, v in fields.items():
            if f not in ("gen_mode", "gen_min_agents"):
                assert v != R.DEFAULTS[f], (name, f)
    assert set(R.CLIPPED) | {"reward_at_goal"} == set(R.UNCLIPPED) == {k for k in R.DEFAULTS if not k.startswith("gen_")}
    assert "reward_at_goal" not in R.CLIPPED                # the clip hides it: held under UNCLIPPED
    # both clip ends act under CLIPPED, neither under UNCLIPPED
    assert R.CLIPPED["reward_clip_hi"] < R.DEFAULTS["reward_at_goal"] and R.CLIPPED["reward_clip_lo"] > R.CLIPPED["reward_collision"]
    assert R.UNCLIPPED["reward_clip_lo"] < R.UNCLIPPED["reward_collision"] and R.UNCLIPPED["reward_at_goal"] < R.UNCLIPPED["reward_clip_hi"]
    # the max-turn clamp acts on the WIDE table, and not on all of it
    turns = np.abs(np.asarray(R.WIDE)[:, 1])
    assert (turns > R.CLIPPED["max_turn_rate"] * R.CLIPPED["dt"]).any() and (turns < R.CLIPPED["max_turn_rate"] * R.CLIPPED["dt"]).any()
    ocfg, ogen = co.default_cfg(6), co.default_gen(6, 6)
    for f, v in R.DEFAULTS.items():
        got = getattr(ogen, rp._GEN[f]) if f in rp._GEN else getattr(ocfg, f)
        assert (tuple(got) if isinstance(v, tuple) else got) == v, f


def test_the_library_is_handed_every_field_of_every_case():
    """make_cfg (the env's side) and replay.oracle_for (the oracle's side) carry the same number in every field of every case, and the
    library's own defaults are DEFAULTS: the host half of 'set on both sides' (no GPU: the library loads without one)"""
    from rl_collision_avoidance_amd.batched_env import make_cfg
    from rl_collision_avoidance_amd.config import EnvConfig

    def env_cfg(N, **over):
        class Cfg(EnvConfig):
            def __init__(self):
                self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
                self.MAX_NUM_OTHER_AGENTS_OBSERVED = N - 1
                EnvConfig.__init__(self)
        return make_cfg(Cfg(), **over)
    plain = env_cfg(6)
    for f, v in R.DEFAULTS.items():
        got = getattr(plain, f)
        assert (tuple(got) if isinstance(v, tuple) else got) == v, f
    assert plain.gen_pool_size == R.DEFAULT_POOL and plain.gen_min_agents == 6
    for case in R.CASES:
        cfg = env_cfg(case.N, **case.over)
        ocfg, ogen = R.oracle_for(case)
        for f in sorted(set(R.DEFAULTS) | {"gen_min_agents", "gen_mode", "gen_pool_size", "dynamics", "num_actions"}):
            want = getattr(ogen, rp._GEN[f]) if f in rp._GEN else getattr(ocfg, f)
            got = getattr(cfg, f)
            if f in ("gen_box_small", "gen_box_large"):
                assert tuple(got) == tuple(want), (case.cid, f)
            else:
                assert got == want, (case.cid, f, got, want)
        assert np.array_equal(np.asarray(cfg.actions)[:cfg.num_actions], np.asarray(ocfg.actions)[:ocfg.num_actions]), case.cid
        for f, v in case.fields.items():                   # ... and it is the set's number, not the default
            got = getattr(cfg, f)
            assert (tuple(got) if isinstance(v, tuple) else got) == v, (case.cid, f)


@pytest.mark.parametrize("cid", [c.cid for c in R.CASES])
def test_every_gpu_case_sees_its_events(cid):
    case = R.BY_ID[cid]
    run = (_topup_run if case.family == "topup" else _run)(cid)[0]
    assert run.t == R.steps_of(case)
    R.assert_events(case, run)
    kinds = {k for k, _, _ in case.plan}
    if case.family == "topup":          # nothing but K-step launches of at most half a ring: no refill launch behind the first fill
        assert kinds <= {"slots", "packed"} and all(K == n and 2 * K <= case.over["gen_lookahead"] for _, K, n in case.plan)
    else:
        assert case.cid.startswith("actor") or kinds == {"single", "slots", "packed"}


@pytest.mark.parametrize("cid", [c.cid for c in NUMERIC])
def test_every_field_decides_something(cid):
    case = R.BY_ID[cid]
    _, first, never = _run(cid)
    print("%s (%d x %d, %d steps): first differing step, 0 = the generated state" % (cid, case.N, case.W, R.steps_of(case)))
    print("    " + ", ".join("%s %d" % (f, first[f]) for f in sorted(first, key=lambda f: (first[f], f))))
    assert not never, (cid, "a default in place of these fields would pass the case", never)
    assert set(first) == set(case.fields)
    want = set(R.UNCLIPPED if "-unclipped-" in cid else R.CLIPPED) | set(R.BOX if "box" in cid else R.RING)
    # (reward_at_goal is hidden by the clip under CLIPPED, reward_clip_hi never reached under UNCLIPPED: by construction)
    assert set(case.fields) == want - {"gen_mode", "reward_clip_hi" if "-unclipped-" in cid else "reward_at_goal"}


def test_goals_and_time_outs_are_seen_per_dynamics_and_form_family():
    seen = {}
    for case in R.CASES:
        if case.family == "topup":                          # (no goal is reached under their time budget)
            continue
        run = _run(case.cid)[0]
        key = (case.family, case.over.get("dynamics", 0))
        s = seen.setdefault(key, {"goal": 0, "timeout": 0})
        s["goal"] += run.seen["goal"]
        s["timeout"] += run.seen["timeout"]
    assert set(seen) == {("tile", 1), ("crowd", 0), ("crowd", 1), ("crowd", 2)}
    for key, s in seen.items():
        assert s["goal"] > 0 and s["timeout"] > 0, (key, s)


# ---- the relay launch's ring top-up: what the cases of tests/test_gpu_topup_oracle.py prove about records only the role can have made ----
@functools.lru_cache(maxsize=None)
def _topup_run(cid):
    """(the case's oracle run, {field: first differing step}, the fields that never differed, agent kinds seen in episodes above R).
    Beside the case's run, one run per field of a top-up wavefront that took THAT field at its default: the same oracle, but a world that
    restarts into an episode above R (a record of the role's making: the first fill holds R) is generated again with the field at its
    default; the run is dropped at its first difference from the case's run -- an output of the step, a flag bit or the state."""
    from oracle import c_oracle as co
    case = R.BY_ID[cid]
    ring = case.over["gen_lookahead"]
    base = R.OracleRun(case)
    live = {f: (R.OracleRun(case), R.oracle_for(case, **{f: R.field_default(f, case.N)})) for f in case.fields}
    first, kinds = {}, collections.Counter()
    for kind, K, n in case.plan:
        _, fed = base.draw(K)
        for t in range(n):
            out = base.step(fed[t])
            fl = base.st.flags.reshape(case.W, case.N)[base.turns() > ring]
            present = (fl & R.F_PRESENT) != 0
            kinds["absent"] += int((~present).sum())
            kinds["static"] += int((present & (((fl >> 8) & 7) == 1)).sum())
            kinds["nonlearning"] += int((present & ((fl & 0x40) == 0)).sum())
            for f in list(live):
                run, (acfg, agen) = live[f]
                obs, rew, done, go = run.step(fed[t])
                again = ((go != 0) & (run.turns() > ring)).astype(np.uint8)
                if again.any():
                    co.generate(acfg, agen, case.seed, run.st, run.ep, again, world_offset=case.offset)
                    obs[again != 0] = co.observe(run.cfg, run.st)[again != 0]
                if _step_differs(out, (obs, rew, done, go), base.st, run.st) or _state_differs(base.st, run.st):
                    first[f] = base.t
                    del live[f]
    return base, first, sorted(live), kinds


@pytest.mark.parametrize("cid", [c.cid for c in TOPUP])
def test_every_field_the_topup_role_loads_decides_something_above_the_first_fill(cid):
    case = R.BY_ID[cid]
    run, first, never, kinds = _topup_run(cid)
    print("%s (%d x %d, %d steps): episodes per world %d .. %d; first differing step of a role with the field at its default"
          % (cid, case.N, case.W, R.steps_of(case), run.turns().min(), run.turns().max()))
    print("    " + ", ".join("%s %d" % (f, first[f]) for f in sorted(first, key=lambda f: (first[f], f))))
    assert not never, (cid, "a top-up role with a default in place of these fields would pass the case", never)
    # every RING field and the time budget, but for what cannot decide by construction (cfg_regimes._topup)
    want = set(R.RING) | {"max_time_ratio"}
    if case.over["gen_min_agents"] == case.N:
        want -= {"gen_min_agents"}
    if case.N == 1:
        want -= {"gen_static_fraction", "gen_nonlearning_fraction"}
    assert set(first) == set(case.fields) == want
    assert all(case.over[f] != R.field_default(f, case.N) for f in case.fields)
    # absent agents where worlds may be smaller than N, scripted (static among them) agents wherever a world has a second agent
    assert (kinds["absent"] > 0) == (case.over["gen_min_agents"] < case.N), (cid, dict(kinds))
    assert (kinds["static"] > 0 and kinds["nonlearning"] > kinds["static"]) == (case.N > 1), (cid, dict(kinds))


def test_the_oracle_of_a_shard_is_the_shards_worlds_of_the_whole_batch():
    """40 worlds at world_offset 300 == worlds 300 .. 339 of 512 worlds at offset 0, bit for bit over the offset case's steps: the
    reference the GPU test holds the role's `world_offset + w` to is the sharded one"""
    from oracle import c_oracle as co
    case = R.BY_ID["topup-clipped-n4x40-offset300"]
    W, N, lo = 512, case.N, case.offset
    cfg, gen = R.oracle_for(case)
    whole, shard = co.State.empty(W, N), co.State.empty(case.W, N)
    ep_whole, ep_shard = np.zeros(W, np.uint32), np.zeros(case.W, np.uint32)
    co.generate(cfg, gen, case.seed, whole, ep_whole)
    co.generate(cfg, gen, case.seed, shard, ep_shard, world_offset=lo)
    rng = np.random.default_rng(case.seed)
    rows = slice(lo * N, (lo + case.W) * N)
    for t in range(R.steps_of(case)):
        a = R._goal_seeking_actions(rng, W, N)
        ow = co.step_autoreset(cfg, gen, case.seed, whole, ep_whole, a)
        os_ = co.step_autoreset(cfg, gen, case.seed, shard, ep_shard, a[lo:lo + case.W], world_offset=lo)
        assert all(np.array_equal(x[lo:lo + case.W], y) for x, y in zip(ow, os_)), t
        assert np.array_equal(whole.f64[:, rows], shard.f64) and np.array_equal(whole.f32[:, rows], shard.f32), t
        assert np.array_equal(whole.flags[rows], shard.flags) and np.array_equal(ep_whole[lo:lo + case.W], ep_shard), t
    assert ep_shard.min() >= 3 * case.over["gen_lookahead"]
    plain = co.State.empty(case.W, N)                       # ... and the offset decides: worlds 0 .. 39 are other worlds
    co.generate(cfg, gen, case.seed, plain, np.zeros(case.W, np.uint32))
    assert _state_differs(plain, shard)
