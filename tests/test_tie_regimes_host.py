"""CPU proof that the hand-placed cases of tests/tie_regimes.py are what they claim to be -- without it tests/test_gpu_tie_regimes.py could
pass vacuously: the two oracles agree bit for bit on every case at every step; every triple straddles its predicate in float64 and 'at'
falls on the side include/cavoid.h and the oracle's comparison name; every tie is a tie of the fast sort key at the steps it claims (and
at no other, where it claims that); the centimetre buckets at exact halves are the ones round-half-to-even defines.  No case is skipped:
one that does not straddle is rebuilt in tie_regimes.py, not dropped."""
import collections

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import cavoid_oracle as po
from tests import tie_regimes as T

GROUP_NAMES = list(T.GROUPS)
HOST_N = (4, 6)          # the tile forms' first shape and the first with absent agents behind four placed ones and a six-agent line


def _python_cfg(group, N):
    over = T.over_of(group)
    kw = {k: (bool(v) if k in ("sort_round_gap", "sort_tie_lateral", "wrap_closed_end", "actions_fp32", "done_agents_collide") else v)
          for k, v in over.items()}
    if "actions" in kw:
        kw["actions"] = np.asarray(kw["actions"], np.float64)
    return po.OracleConfig(max_agents=N, max_other_agents_observed=T.M_of(group, N), **kw)


@pytest.mark.parametrize("name", GROUP_NAMES)
def test_the_two_oracles_agree_bitwise_on_every_case(name):
    """tests/test_oracle.py's criterion (_cross): observations, rewards, done, game_over and the whole state, bit for bit, at every step --
    the plain step, no restarts: every hand-placed world runs on past its last learner"""
    N = 4
    group = T.GROUPS[name]
    run = T.Run.of(name, N)
    pcfg = _python_cfg(group, N)
    ccfg, _ = T.oracle_for(group, N)
    st = run.start.copy()
    placed = [T.world_index(k) for k, _ in run.worlds()]
    assert len(placed) == len(T.worlds_of(group, N)) > 0
    worlds = {}
    for w in placed:
        sl = slice(w * N, (w + 1) * N)
        worlds[w] = po.world_from_arrays(st.f64[:, sl], st.f32[:, sl], st.flags[sl], pcfg)
    o0 = co.observe(ccfg, st)
    for w, wd in worlds.items():
        assert np.array_equal(wd.observe(), o0[w]), (name, w)
    for t in range(T.STEPS):
        obs, rew, done, go = co.step(ccfg, st, run.acts[t])
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


@pytest.mark.parametrize("N", HOST_N)
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_every_triple_straddles_and_at_takes_the_named_side(name, N):
    run = T.Run.of(name, N)
    triples = collections.defaultdict(dict)
    for k, w in run.worlds():
        if w.probe is not None:
            assert run.eps[max(w.probe.step, 0)][T.world_index(k)] == 0 or w.probe.step < 0, (w.name, "restarted before its probe")
            triples[w.probe.triple][w.probe.role] = (T.read(run, k, w.probe), w)
    for tid, roles in triples.items():
        at, w = roles["at"]
        above = roles["above"][0]
        assert at != above or w.probe.at_side == "above", (tid, at, above)
        if "below" in roles:
            below = roles["below"][0]
            assert below != above, (tid, "does not straddle", below, above)
            assert at == (below if w.probe.at_side == "below" else above), (tid, "at", at, "below", below, "above", above)
            assert set(roles) == {"below", "at", "above"}
        else:
            assert w.probe.at_side is None and at != above, (tid, at, above)
    with_probes = [w for w in T.worlds_of(T.GROUPS[name], N) if w.probe is not None]
    assert sum(len(r) for r in triples.values()) == len(with_probes)              # none left out


def test_known_answers_of_the_threshold_cases():
    """the numbers the cases are built on, from the oracle: -0.25 and flag 4 at gap 0.0, the close penalty -0.1 + 0.5 * 0.25 at gap 0.25,
    reward 1.0 and flag 1 at d^2 = thr^2, flag 2 at t_remaining = 0.0; one ulp off: 0.0 (the close penalty for the missed collision)"""
    run = T.Run.of("main", 4)
    got = {w.name: T.read(run, k, w.probe) for k, w in run.worlds() if w.probe is not None}
    for k in (1, 4):
        assert got["P1-cd0-k%d-at" % k] == (True, -0.25) and got["P1-cd0-k%d-below" % k] == (True, -0.25)
        assert got["P1-cd0-k%d-above" % k] == (False, -0.1)                   # the close penalty at gap 1 ulp: -0.1 + 0.5 * 2^-52
        assert got["P2-k%d-at" % k] == (0.025,) == got["P2-k%d-below" % k] and got["P2-k%d-above" % k] == (0.0,)
        assert got["P4-k%d-at" % k] == (True, 1.0) and got["P4-k%d-above" % k] == (False, 0.0)
        assert got["P5-k%d-at" % k] == (True, 1) and got["P5-k%d-above" % k] == (False, 0)
    run = T.Run.of("horizon", 4)
    got = {w.name: T.read(run, k, w.probe) for k, w in run.worlds() if w.probe is not None}
    assert got["P3-one-k1-at"] == (1.0, (0.25, 0.0, 0.0)) and got["P3-one-k1-above"] == (0.0, (0.0, 0.0, 0.0))
    assert got["P3-two-k4-at"] == (2.0, (0.25, 0.125, 0.0)) and got["P3-two-k4-above"] == (1.0, (0.125, 0.0, 0.0))
    for closed, name in ((False, "pi-open"), (True, "pi-closed")):
        run = T.Run.of(name, 4)
        for k, w in run.worlds():
            if w.probe is not None and w.probe.role == "at":
                h = run.states[w.probe.step].f64[2, T.world_index(k) * 4]
                assert h == (np.pi if closed else -np.pi), (w.name, h)          # exactly +-pi, the sign the switch names


@pytest.mark.parametrize("N", HOST_N)
def test_half_centimetre_buckets_round_half_to_even(N):
    """expected from the definition, written out in tie_regimes.py beside HALVES: 12.5 -> 12, 37.5 -> 38, 62.5 -> 62, -12.5 -> -12"""
    assert {h: (np.rint(h * 100.0), way) for h, (_, _, way) in T.HALVES.items()} == {
        0.125: (12.0, "down"), 0.375: (38.0, "up"), 0.625: (62.0, "down"), -0.125: (-12.0, "up")}
    assert all(float(h * 100.0) * 2 == round(h * 200) for h in T.HALVES)            # x 100 is exact: a real half
    run = T.Run.of("main", N)
    M = T.M_of(run.group, N)
    seen = 0
    for k, w in run.worlds():
        if w.order is not None:
            row = run.row(k, w.probe.step, w.probe.host)
            assert T.slot_radii(row, M) == T.expected_slots(w, w.order, M), (w.name, T.slot_radii(row, M))
            seen += 1
    assert seen == len(T.HALVES) * 2 * 3


def _keys(run, k, world, step):
    """per tied neighbour: (centimetre bucket, float64 lateral ry * tx - rx * ty, float64 gap) as the host sees it in the state after `step`"""
    st = run.state(step)
    base = T.world_index(k) * run.N
    h = base + world.tie.host
    tx, ty = float(st.f32[0, h]) - st.f64[0, h], float(st.f32[1, h]) - st.f64[1, h]
    out = []
    for j in world.tie.group:
        rx, ry = st.f64[0, base + j] - st.f64[0, h], st.f64[1, base + j] - st.f64[1, h]
        gap = np.sqrt(rx * rx + ry * ry) - float(st.f32[2, h]) - float(st.f32[2, base + j])
        out.append((np.rint(gap * 100.0), ry * tx - rx * ty, gap))
    return out


@pytest.mark.parametrize("N", HOST_N)
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_every_tie_is_a_tie(name, N):
    run = T.Run.of(name, N)
    exact_gap = T.over_of(run.group).get("sort_round_gap", 1) == 0
    ties = 0
    for k, w in run.worlds():
        if w.tie is None:
            continue
        ties += 1
        radii = [w.agents[j].r for j in w.tie.group]
        assert len(set(radii)) == len(radii), w.name                         # each tied neighbour identifiable by its radius
        for step in range(-1, T.STEPS):
            assert step < 0 or run.eps[step][T.world_index(k)] == 0, (w.name, "restarted")
            keys = _keys(run, k, w, step)
            bucket = {b for b, _, _ in keys}
            lat64 = {l for _, l, _ in keys}
            lat32 = {np.float32(l).tobytes() for _, l, _ in keys}
            gap64 = {g for _, _, g in keys}
            gap32 = {np.float32(g).tobytes() for _, _, g in keys}
            claimed = step in w.tie.steps
            if w.tie.kind == "full":
                fast_tie = len(bucket) == 1 and len(lat32) == 1
                assert fast_tie == claimed, (w.name, step, keys)
                assert not claimed or len(lat64) == 1, (w.name, step, keys)
            elif w.tie.kind == "f32":
                assert len(bucket) == 1 and len(lat32) == 1 and len(lat64) == len(keys), (w.name, step, keys)
            elif w.tie.kind == "gap64":
                assert len(gap64) == 1 and len(lat64) == len(keys), (w.name, step, keys)
            elif w.tie.kind == "gap32":
                assert len(gap32) == 1 and len(gap64) == len(keys), (w.name, step, keys)
            else:
                raise AssertionError(w.tie.kind)
            if exact_gap and w.tie.kind in ("gap64", "gap32"):
                assert len(gap32) == 1                                        # the exact-gap key (float32 gap, no lateral) coincides
    assert ties >= 1                                                          # (every group has the line of N at least)


def test_the_ties_decide_what_they_claim():
    """slot identity, from the cases' own docstrings (closest_last, every neighbour kept unless said): the index, the float64 lateral, the
    exact gap and the cut really decide"""
    def slots(name, wname, step=0, N=4):
        run = T.Run.of(name, N)
        k, w = next((k, w) for k, w in run.worlds() if w.name == wname)
        return T.slot_radii(run.row(k, step, w.tie.host), T.M_of(run.group, N)), w
    R1, R2, R3 = [float(np.float32(r)) for r in (T.R1, T.R2, T.R3)]
    assert slots("main", "T1-two")[0] == (R1, R2, 0.0)                           # index order
    assert slots("main", "T1-three")[0] == (R1, R2, R3)
    assert slots("main", "T4-f32-lateral")[0] == (R2, R1, 0.0)                   # the smaller float64 lateral first, against the index
    assert slots("m2", "T2-cut")[0] == (R2, 0.375)                               # the cut between the tied 1 and 2: 2 kept
    assert slots("near", "T1-three")[0] == (R1, R2, R3)                          # T3: near to far, full ties in index order
    assert slots("near-m2", "T2-cut")[0] == (0.375, R2)
    for swapped in ("", "-swapped"):                                             # (agents 1 and 2 exchanged: the same radii in the same slots)
        assert slots("main", "T4-f32-lateral" + swapped)[0] == (R2, R1, 0.0)
        assert slots("exact-gap", "T5-gap-bit-equal" + swapped)[0] == (0.5, 0.25, 0.0)     # lateral -1.5 before +1.5
        assert slots("exact-gap", "T5-gap-f32-equal" + swapped)[0] == (0.5, 0.25, 0.0)     # the larger float64 gap first
    assert slots("index-tie", "T1-two")[0] == (R1, R2, 0.0)
    for step in range(T.STEPS):
        assert slots("main", "T7-persists", step)[0] == (R1, R2, 0.0)
    assert slots("main", "T8-appears", 2)[0] == (R1, R2, 0.0)
    got, w = slots("main", "line-6", 0, 6)                                        # pairs by agent index, not in ring order from agent 3
    assert got == tuple(float(np.float32(w.agents[i].r)) for i in (5, 2, 4, 0, 1))
