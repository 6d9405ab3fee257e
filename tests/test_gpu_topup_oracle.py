"""The top-up wavefront of the relay launch (`relay_topup`, csrc/cavoid_relay.hpp) held to the float64 oracle WHERE ITS RECORDS ARE READ.
The role regenerates consumed slots of the look-ahead rings from its own loads of the kernel arguments (the generator fields, the time
budget, `world_offset`, the episode counters, the ring bookkeeping); a record it makes is read only once its world has used up the R
episodes of the first fill.  The `topup-` cases of tests/cfg_regimes.py run nothing but relay launches of at most R / 2 steps behind the
reset, with the generator and the step off their default numbers and a time budget that restarts worlds every few steps, until EVERY
world has read records three rings deep -- every step of every launch against the oracle (tests/test_cfg_regimes_host.py proves on
the CPU that within those steps each field the role loads decides something in records only the role can have made).  Beside them: every
consumer count, a resume from a checkpoint, and episode counters that pass 2^32.

`cavoid_ahead_info` counts the refill launches: 1 at the end of every case -- the first fill and nothing else."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import cfg_regimes as R

pytestmark = pytest.mark.gpu

TOPUP = R.select("topup-")


def _env(case, **over):
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.config import EnvConfig

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = case.N
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = case.N - 1
            EnvConfig.__init__(self)
    return BatchedCollisionAvoidanceEnv(case.W, Cfg(), device="cuda:0", world_offset=case.offset, seed=case.seed, **dict(case.over, **over))


@pytest.mark.parametrize("cid", [c.cid for c in TOPUP])
def test_every_record_the_role_makes_is_read_against_the_oracle(cid):
    case = R.BY_ID[cid]
    env = _env(case)
    run = R.drive_gpu(case, env, *case.forms)               # (every launch asserts the RELAY form)
    R.assert_events(case, run)
    assert env.lookahead_info[0] == 1, env.lookahead_info   # the first fill and nothing else
    env.close()


def _budget_rule(case, topup):
    """(refill launches, budget) behind the reset and behind every launch of the case by the host's rule (cavoid_ahead_prepare /
    cavoid_ahead_consumed): the reset fills the rings and consumes one episode; a launch with the role needs a budget of K and leaves
    R - K; one without it needs K + 1, refills when short of that, and consumes K"""
    ring = case.over["gen_lookahead"]
    refills, budget = 1, ring - 1
    seq = [(refills, budget)]
    for _, K, _ in case.plan:
        if topup:
            assert budget >= K
            budget = ring - K
        else:
            if budget < K + 1:
                refills, budget = refills + 1, ring
            budget -= K
        seq.append((refills, budget))
    return seq


@pytest.mark.parametrize("nc", [1, 2, 4])
def test_every_consumer_count_against_the_oracle(nc, monkeypatch):
    """the role is the wavefront behind the 3 + nc of the step: its place in the workgroup moves with the consumer count, and whether the
    launch carries it at all is the occupancy calculator's answer for that shape.  Either way the results are the oracle's; the refill
    launches follow EXACTLY one of the two patterns of the host's rule: with the role none behind the first fill, without it one in
    front of every launch that finds less than K + 1 episodes covered"""
    case = R.BY_ID["topup-clipped-n4x40"]
    monkeypatch.setenv("CAVOID_RELAY_CONSUMERS", str(nc))
    env = _env(case)
    monkeypatch.delenv("CAVOID_RELAY_CONSUMERS", raising=False)
    seen = []
    run = R.drive_gpu(case, env, "QUAD", ("RELAY", nc), after_launch=lambda launch: seen.append(env.lookahead_info))
    R.assert_events(case, run)
    with_role, without = _budget_rule(case, True), _budget_rule(case, False)
    assert with_role[1] != without[1]                       # (the first launch already tells the two apart)
    carried = seen[0] == with_role[1]
    print("CAVOID_RELAY_CONSUMERS=%d: the launches %s the top-up wavefront; refill launches %d" % (nc, "carry" if carried else "run without", seen[-1][0]))
    assert seen == (with_role if carried else without)[1:], (nc, seen)
    env.close()


def test_a_resumed_env_fills_its_rings_from_the_checkpoints_episodes():
    """24 launches, a checkpoint, a second look-ahead env loaded from it: its first fill starts from non-zero episode counters that differ
    from world to world, and its first launch already carries the role.  24 more launches on both: bitwise the same, both the oracle's,
    and one refill launch each"""
    case = R.BY_ID["topup-clipped-n4x40"]
    half = len(case.plan) // 2
    env = _env(case)
    run = R.drive_gpu(case._replace(plan=case.plan[:half]), env, *case.forms)
    sd = env.state_dict()
    at = sd["episode"].cpu().numpy().view(np.uint32)
    assert np.array_equal(at, run.ep) and at.min() >= case.over["gen_lookahead"] and len(set(at.tolist())) > 4
    resumed = _env(case)
    resumed.load_state_dict(sd)
    assert resumed.lookahead_info == (0, 0)                 # nothing filled yet
    R.drive_plan(case, env, run, case.plan[half:], *case.forms, twin=resumed, twin_form="RELAY")
    R.assert_events(case, run)
    assert env.lookahead_info[0] == 1 and resumed.lookahead_info[0] == 1
    env.close(); resumed.close()


def test_episode_counters_that_pass_2_to_the_32():
    """`seed(s, episode)` a few episodes short of 2^32, one-step episodes, 12 launches of 4 steps on rings of 8: the role's uint32 ring
    arithmetic -- (int32)(hi - episode), the slot e & (R - 1), and the bookkeeping value 0xFFFFFFFF, which is also 'nothing filled yet' --
    across the wrap.  The first launch enters at episode[w] + 1 and tops up to episode[w] + 9: 0xFFFFFFFF in the worlds that start at
    2^32 - 10.  Against the oracle, and bitwise against an env that generates inside the step.
    Known and benign (beside the role): in such a world the NEXT launch's role takes 0xFFFFFFFF for 'nothing filled' and makes
    episodes ep + 1 .. ep + R again, slots the launch's own loader reads among them -- the one place where the role writes what its launch
    reads.  The bytes are those already there (the generator is a function of seed, world and episode), which is what this test holds."""
    base = R.BY_ID["topup-clipped-n4x40"]
    launches, K = 12, 4
    case = base._replace(cid="topup-wrap-n4x40", over=dict(base.over, max_time_ratio=1e-9), plan=base.plan[:launches])
    start = (2 ** 32 - 10 - np.arange(case.W) % 7).astype(np.uint32)
    assert ((start + np.uint32(1 + case.over["gen_lookahead"])) == np.uint32(0xFFFFFFFF)).any()
    env, instep = _env(case), _env(case, gen_lookahead=0)
    run = R.drive_gpu(case, env, "QUAD", "RELAY", start_episode=start, twin=instep)
    want = (39 - np.arange(case.W) % 7).astype(np.uint32)    # 1 (the reset) + 48 (one per step) beyond the start, modulo 2^32
    assert launches * K == 48 and np.array_equal(run.ep, want)
    assert np.array_equal(env.episode.cpu().numpy().view(np.uint32), want)
    assert (run.turns() == launches * K).all() and launches * K >= 3 * case.over["gen_lookahead"]
    assert env.lookahead_info[0] == 1, env.lookahead_info
    env.close(); instep.close()
