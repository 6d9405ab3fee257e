"""CPU proof that the placed cases of tests/orca_regimes.py are what they claim to be -- without it tests/test_gpu_orca_regimes.py could
pass vacuously.  For every case: the host's trace (oracle/cavoid_oracle.py's hook) holds the named decisions on the named sides at the
named step, in every placement and with every other slot of the world filled by far static agents, whose lines never bind (the host's
action is the same bit for bit); the two oracles agree bit for bit on the run.  For the branch cases: the trace is identical and the
action moves by less than 1e-10 under 32 sign patterns of +-1e-12 on every coordinate and heading (so the GPU comparison at 1e-9 is a
statement about the kernel, not about conditioning -- and so is every later step of the placed world's life), and flipping the one
decision moves the action by more than 1e-3.  For the exact cases: the deciding quantity of `at` IS the threshold, below and above fall
on opposite sides, and their displacement is the smallest that does.  Coverage: every named decision on both sides, in both groups."""
import collections
import math

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import cavoid_oracle as po
from tests import orca_regimes as R

BRANCH_GROUPS = ("default", "off")
HOST_N = 8               # every case fits (at most 7 agents) and every placement has at least one filler


def _cases(names=R.GROUPS):
    return [(g, c) for g in names for c in R.GROUPS[g].cases]


def _ids(pairs):
    return ["%s:%s" % (g, c.name) for g, c in pairs]


ALL = _cases()
BRANCH = [(g, c) for g, c in _cases(BRANCH_GROUPS) if c.exact is None]


def test_the_hook_names_exactly_the_listed_decisions():
    """every _br site of the oracle is in DECISIONS and the other way round; the names of a case's claims are among them"""
    import inspect
    import re
    src = inspect.getsource(po)
    sites = set()
    for m in re.finditer(r'_br\(hook, (?:\("dir" if direction_opt else "lp"\)|pre) \+ "(\.\w+)"', src):
        sites.update(("lp" + m.group(1), "dir" + m.group(1)))
    sites.update(re.findall(r'_br\(hook, "([\w.]+)"', src))
    # the direction-optimising programme never clamps to the preferred velocity or clips it to the disc, the first one never picks an end
    assert sites == set(R.DECISIONS), sites ^ set(R.DECISIONS)
    for g, c in ALL:
        assert all(name in R.DECISIONS for name, _ in c.claims), c.name
        assert len({a.r for a in c.agents}) == len(c.agents), (c.name, "every agent its own radius")
        assert c.agents[0].pol == R.ORCA


@pytest.mark.parametrize("g,case", ALL, ids=_ids(ALL))
def test_the_trace_holds_the_claims_in_every_placement(g, case):
    cfg = R.python_cfg(R.GROUPS[g], len(case.agents))
    t0, a0 = R.trace_of(case.agents, 0, case.step, cfg)
    assert a0 is not None, "the host is done before the step"
    for claim in case.claims:
        assert t0.has(*claim), (case.name, claim, t0.seen)
        assert not R.unreachable(*claim)
    for N in (HOST_N, 21, 64):
        cfgN = R.python_cfg(R.GROUPS[g], N)
        for c in (0, 3):                                     # (case number 3: the rest of the first placement absent)
            for p in R.layouts(case, c, N):
                agents = [a for a in p.agents if a is not None]
                assert all(a is not None for a in p.agents[:len(agents)])             # present agents are contiguous
                t, a = R.trace_of(agents, p.host, case.step, cfgN)
                for claim in case.claims:
                    assert t.has(*claim), (case.name, N, p.variant, claim)
                assert np.array_equal(a, a0), (case.name, N, p.variant, "a far static agent binds", a, a0)


@pytest.mark.parametrize("name", list(R.GROUPS))
def test_the_two_oracles_agree_bitwise_on_every_case(name):
    """tests/test_oracle.py's criterion: observations, rewards, done, game_over and the whole state, bit for bit, at every step of the
    plain step (no restarts: every placed world runs on past its last learner)"""
    N = HOST_N
    group = R.GROUPS[name]
    run = R.Run.of(name, N)
    pcfg = R.python_cfg(group, N)
    st = run.start.copy()
    worlds = {}
    for w, _ in run.placed():
        sl = slice(w * N, (w + 1) * N)
        worlds[w] = po.world_from_arrays(st.f64[:, sl], st.f32[:, sl], st.flags[sl], pcfg)
    assert len(worlds) == 3 * len(group.cases) > 0
    o0 = co.observe(run.cfg, st)
    for w, wd in worlds.items():
        assert np.array_equal(wd.observe(), o0[w]), (name, w)
    for t in range(R.STEPS):
        obs, rew, done, go = co.step(run.cfg, st, run.acts[t])
        for w, wd in worlds.items():
            n = len(wd.agents)
            pobs, prew, pgo, info = wd.step({i: run.acts[t, w, i] for i in range(n)})
            tag = (name, t, w)
            assert np.array_equal(pobs, obs[w]), tag
            assert np.array_equal(prew, rew[w, :n]) and pgo == bool(go[w]), tag
            assert [info["which_agents_done"][i] for i in range(n)] == list(done[w, :n].astype(bool)), tag
            f64, f32, fl = po.world_to_arrays(wd)
            sl = slice(w * N, (w + 1) * N)
            assert np.array_equal(f64, st.f64[:, sl]) and np.array_equal(fl, st.flags[sl]) and np.array_equal(f32, st.f32[:, sl]), tag


def test_the_placed_worlds_are_met_and_end_as_planned():
    """in the auto-reset run a branch world is still in its first episode at its step and is restarted one step later; an exact world is
    over after step 1; the three placements of the cases take every position of a wavefront of three and of two"""
    for name in R.GROUPS:
        run = R.Run.of(name, HOST_N)
        for w, p in run.placed():
            s = p.case.step
            if name == "exact":
                assert run.eps[0][w] == 1, (p.case.name, "not over after its step")
                continue
            assert run.eps[s - 1][w] == 0, (p.case.name, "restarted before its step")
            assert run.eps[s][w] == 1, (p.case.name, "runs on after the step behind its decision")
        seen = collections.defaultdict(set)
        for w, p in run.placed():
            seen[p.variant].add((w % 3, w % 2))
        if len(R.GROUPS[name].cases) >= 6:
            for v in range(3):
                assert {m3 for m3, _ in seen[v]} == {0, 1, 2} and {m2 for _, m2 in seen[v]} == {0, 1}, (name, v)
        where = collections.defaultdict(list)
        for w, p in run.placed():
            where[p.case.name].append(w)
        for case, ws in where.items():                      # ... and so do the three placements of every single case
            assert {w % 3 for w in ws} == {0, 1, 2} and {w % 2 for w in ws} == {0, 1}, (name, case, ws)


@pytest.mark.parametrize("g,case", BRANCH, ids=_ids(BRANCH))
def test_a_branch_case_is_well_conditioned_and_its_decision_matters(g, case):
    cfg = R.python_cfg(R.GROUPS[g], len(case.agents))
    ok, why = R.conditioned(case.agents, 0, case.step, cfg)
    assert ok, (case.name, why)
    for name, side in case.claims:
        moved = R.flip_moves(case.agents, 0, case.step, cfg, name, side)
        assert moved > R.FLIP_MOVES, (case.name, name, side, moved)
    assert case.inexact == any(a.px * 8.0 != round(a.px * 8.0) or a.py * 8.0 != round(a.py * 8.0) for a in case.agents)


@pytest.mark.parametrize("name", BRANCH_GROUPS)
def test_the_whole_life_of_a_branch_world_is_well_conditioned(name):
    """the GPU test compares every step until the world is restarted: the C oracle's float64 state after each of them moves by less than
    1e-10 (flags not at all) under the same 32 patterns, all placed worlds of the batch perturbed at once"""
    N = HOST_N
    run = R.Run.of(name, N)
    placed = [w for w, _ in run.placed()]
    cols = np.concatenate([np.arange(w * N, (w + 1) * N) for w in placed])
    present = (run.start.flags[cols] != 0) & np.repeat([p.case.exact is None for _, p in run.placed()], N)     # (not the equalities)

    def life(st):
        out = []
        for t in range(R.STEPS):
            co.step(run.cfg, st, run.acts[t])
            out.append((st.f64[:3, cols].copy(), st.flags[cols].copy()))
        return out
    base = life(run.start.copy())
    rng = np.random.default_rng(4321)
    for k in range(R.PATTERNS):
        st = run.start.copy()
        st.f64[:3, cols] += rng.choice([-R.PERTURB, R.PERTURB], (3, len(cols))) * present
        for t, ((a, fa), (b, fb)) in enumerate(zip(base, life(st))):
            live = np.repeat([t <= p.case.step for _, p in run.placed()], N)          # steps 1 .. step + 1 of the world's life
            assert np.array_equal(fa[live], fb[live]), (name, k, t)
            d = np.abs(a - b)[:, live]
            assert float(d.max()) < 1e-10, (name, k, t, float(d.max()), run.placed()[int(np.argmax(d.max(axis=0))) // N][1].case.name)


# ---- exact cases -----------------------------------------------------------------------------------------------------------------------
def test_exact_triples_sit_on_the_threshold_and_straddle_it():
    cases = {c.name: c for c in R.GROUPS["exact"].cases}
    for tid, (build, quantity, decision, pred) in R.TRIPLES.items():
        q = R.QUANTITY[quantity]
        below, at, above = [cases["X-%s-%s" % (tid, role)] for role in ("below", "at", "above")]
        assert q(at.agents) == 0.0 and at.claims == ((decision, pred(0.0)),)
        assert q(below.agents) < 0.0 < q(above.agents), (tid, q(below.agents), q(above.agents))
        assert dict(below.claims)[decision] != dict(above.claims)[decision], tid
        assert dict(at.claims)[decision] == dict(below.claims if pred(-1.0) == pred(0.0) else above.claims)[decision]
        for sign in (-1, 1):                                 # the smallest displacement: one step less leaves the quantity at 0
            k = R.smallest_displacement(build, quantity, sign)
            assert q(build(sign * k)) != 0.0 and all(q(build(sign * j)) == 0.0 for j in range(k))
            assert [tuple(a) for a in build(sign * k)] in ([tuple(a) for a in below.agents], [tuple(a) for a in above.agents])
        for c in (below, at, above):                         # exactly representable: grid numbers, ulps of them, heading exactly 0
            assert all(a.heading == 0.0 and a.t == R.ONE_DT for a in c.agents), c.name
    assert R.smallest_displacement(R._det, "det", 1) > 1    # a shift of one denormal ulp underflows in the products
    # the solved velocity of the coincident lines is exactly zero (act.moving false): a decision no search reached
    cfg = R.python_cfg(R.GROUPS["exact"], 4)
    t, a = R.trace_of(cases["X-num-at"].agents, 0, 1, cfg)
    assert t.has("act.moving", False) and t.has("lp.parallel", True) and tuple(a) == (0.0, 0.0)
    for name in ("X-parallel-skipped", "X-squeezed"):
        assert cases[name].exact is None and len(cases[name].claims) >= 2


# ---- coverage --------------------------------------------------------------------------------------------------------------------------
def _table(name):
    rows = collections.OrderedDict(((d, s), []) for d in R.DECISIONS for s in (True, False))
    for c in R.GROUPS[name].cases:
        for claim in c.claims:
            rows[claim].append(c)
    return rows


@pytest.mark.parametrize("name", BRANCH_GROUPS)
def test_every_decision_is_covered_on_both_sides(name):
    assert len(R.UNREACHABLE) <= 3 and all(d in R.DECISIONS and sides and why for d, (sides, why) in R.UNREACHABLE.items())
    rows = _table(name)
    print("\ngroup %s: decision, side -> cases at step 1 (x: inexact coordinates) | at step 3" % name)
    for (d, s), cases in rows.items():
        first = ["%s%s" % (c.name, "x" if c.inexact else "") for c in cases if c.step == 1]
        third = ["%s%s" % (c.name, "x" if c.inexact else "") for c in cases if c.step == 3]
        print("  %-18s %-5s %s | %s%s" % (d, s, " ".join(first) or "-", " ".join(third) or "-", "   not reachable with a margin" if R.unreachable(d, s) else ""))
    no_step3 = []
    for d in R.DECISIONS:
        for s in (True, False):
            if R.unreachable(d, s):
                assert not rows[(d, s)], (d, s, "listed as unreachable and reached")
                continue
            if (d, s) in R.FLIP_IS_A_NO_OP:                  # traced, and its flip moves nothing at all
                met = 0
                for c in R.GROUPS[name].cases:
                    cfg = R.python_cfg(R.GROUPS[name], len(c.agents))
                    if c.step == 1 and R.trace_of(c.agents, 0, 1, cfg)[0].has(d, s):
                        assert R.flip_moves(c.agents, 0, 1, cfg, d, s) == 0.0, (c.name, d, s)
                        met += 1
                assert met >= 1, (name, d, s)
                continue
            assert any(c.step == 1 for c in rows[(d, s)]), (name, d, s, "no case meets it at step 1")
        both = rows[(d, True)] + rows[(d, False)]
        if d in R.UNREACHABLE and len(R.UNREACHABLE[d][0]) == 2:
            continue
        assert any(c.inexact and c.step == 1 for c in both), (name, d, "no side with inexact coordinates")
        if not any(c.step == 3 for c in both):
            no_step3.append(d)
    print("  no case at step 3:", no_step3 or "none")
    assert sorted(no_step3) == sorted(R.NO_STEP3[name])
    cfg = R.python_cfg(R.GROUPS[name], 8)
    for d in no_step3:                                       # only decisions whose cases end the host's episode at step 1: a collision
        for c in rows[(d, True)] + rows[(d, False)]:
            w = R.world_of(c.agents, cfg)
            w.step({i: a.act for i, a in enumerate(c.agents)})
            assert w.agents[0].in_collision, (d, c.name)


@pytest.mark.parametrize("name", BRANCH_GROUPS)
def test_the_host_on_its_goal_is_an_equality_and_matters(name):
    """gn == 0 and speed == 0 exactly (no margin can hold them, so the +-1e-12 test does not apply): one ulp off the goal the host is
    off it, and each of the two decisions flipped moves the action (a division by zero counts)"""
    case = next(c for c in R.GROUPS[name].cases if c.name == "on-goal")
    cfg = R.python_cfg(R.GROUPS[name], len(case.agents))
    host = case.agents[0]
    assert (host.px, host.py) == (float(host.gx), float(host.gy)) and host.heading != 0.0
    t, a = R.trace_of(case.agents, 0, 1, cfg)
    assert t.has("act.off_goal", False) and t.has("act.moving", False) and tuple(a) == (0.0, 0.0)
    off = [host._replace(px=float(np.nextafter(host.px, 2.0)))] + list(case.agents[1:])
    t, a = R.trace_of(off, 0, 1, cfg)
    assert t.has("act.off_goal", True) and t.has("act.moving", True)
    for claim in case.claims:
        assert R.flip_moves(case.agents, 0, 1, cfg, *claim) > R.FLIP_MOVES, claim


def test_exact_group_shows_the_unreached_sides():
    """what the branch groups list as unreachable by search is either reached by an exact case or stays on the list"""
    rows = _table("exact")
    assert rows[("lp.parallel_out", True)] and rows[("lp.parallel_out", False)] and rows[("pen.parallel", True)] and rows[("pen.same_dir", False)]
