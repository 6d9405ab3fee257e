#!/usr/bin/env python
"""The GA3C actor loop of CROWD worlds (17..64 agents) with the weight_sharing network, K env steps per hipGraph replay: the ONE launch of
`capture_fused_crowd_ws(K)` (`cavoid_crowd_actor_run_ws` -> crowd_ws_rollout_kernel: the ring form of the weight_sharing pass on the tile's
live rows, action draw, crowd env step, Experience bookkeeping per tile inside one kernel) against the path of before, `capture(K)` of
`step()` (per env step the weight_sharing policy kernel -- the ring kernel above 19 observed neighbours --, then `cavoid_step_push`), in the
same process on the same library.

Two twin envs / rollouts / networks (same seeds: their trajectories are bit-identical) are built the way `ga3c.train` builds them -- a
fresh scenario per episode from the generator inside the step, 2..N agents per world, the default rollout settings -- and replay their
graphs one after the other, each replay between two HIP events; the order of the two paths alternates from replay to replay.  Every
configuration is warmed up on both paths, then timed in two passes: the table gives each path's median per pass and over both in us per
ENV STEP (replay time / K), their ratio, and the spread -- the larger of the two paths' |median of pass 1 - median of pass 2|, what a
repeat of the SAME path differs by.  Actors only: no drain, no trainer (a whole training run with --fused-crowd-ws-actor is a measurement
of its own).

    python tools/crowdwsactorbench.py [--steps 1200] [--out profiles/crowd_ws_actor_timing.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
from rl_collision_avoidance_amd.config import EnvConfig
from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
from rl_collision_avoidance_amd.ga3c.policy_kernel import MAX_OTHERS_WS, FusedPolicy
from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout

# agents per world x worlds x observed neighbours: WS-8 (ga3c.train --arch weight_sharing --observed 7 --sort-method closest_first) in
# 20-agent worlds, and every neighbour observed on the ring handle at 32 and 64 agents per world
SHAPES = [(20, 2048, 7), (32, 1024, 31), (64, 512, 63)]
KS = (4, 16)                                       # env steps per replay: ga3c.train's default, and a long launch
MIXES = (0.0, 0.5)                                 # ga3c.train --scripted-fraction (its default --static-fraction / --rvo-fraction)
PATHS = ("fused crowd weight_sharing actor kernel", "one launch per phase")


def make(N, W, M, K, scripted, fused):
    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            self.SCRIPTED_AGENT_FRACTION = scripted
            self.SCRIPTED_STATIC_FRACTION = 0.34
            self.SCRIPTED_RVO_FRACTION = 0.33 if scripted > 0 else 0.0
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = M
            EnvConfig.__init__(self)
            self.AGENT_SORTING_METHOD = "closest_first"
    cfg = Cfg()
    env = BatchedCollisionAvoidanceEnv(W, cfg, device="cuda:0", seed=3, gen_min_agents=2, gen_pool_size=0)
    torch.manual_seed(1234)
    pol = FusedPolicy(NetworkVP_rnn(cfg, seed=0, arch="weight_sharing").to("cuda:0"), seed=77, ws_crowd=M > MAX_OTHERS_WS)
    time_max = int(getattr(cfg, "TIME_MAX", int(4 / cfg.DT)))
    roll = BatchedRollout(env, pol, reflush_done=False, ring_len=max(time_max + 2 + K + 8, 2 * (time_max + 2) + 8))
    roll.reset()
    if fused:
        assert roll.crowd_ws_fused_available, roll.crowd_ws_fused_unavailable_reason
        roll.capture_fused_crowd_ws(K)
    else:
        assert not roll.fused_available
        roll.capture(K)
    return env, pol, roll


def timed_replay(roll):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    roll.replay(1)
    e1.record()
    return e0, e1


def bench(N, W, M, K, scripted, replays, warmup):
    rolls = [make(N, W, M, K, scripted, True), make(N, W, M, K, scripted, False)]
    for _ in range(warmup):
        for _, _, roll in rolls:
            roll.replay(1)
    torch.cuda.synchronize()
    us = []                                                # us[pass][path]: us per env step of every timed replay of that pass
    for _ in range(2):
        events = ([], [])
        for k in range(replays):
            for which in ((0, 1) if k % 2 == 0 else (1, 0)):
                events[which].append(timed_replay(rolls[which][2]))
        torch.cuda.synchronize()
        us.append([[e0.elapsed_time(e1) * 1e3 / K for e0, e1 in ev] for ev in events])
    (ea, _, a), (eb, _, b) = rolls
    # (the value / action rings of rows that need no action are never read and differ by design: the fused kernel hands those rows 0, the
    #  whole-batch policy launch of this batch size -- no row list below 65 536 rows -- its output)
    same = (torch.equal(a.obs, b.obs) and torch.equal(a.emit_t, b.emit_t) and torch.equal(a.x, b.x) and torch.equal(a.ret, b.ret)
            and all(torch.equal(u, v) for u, v in zip(ea.get_state(), eb.get_state())))
    episodes = [int(r.ep_count[0].item()) for _, _, r in rolls]
    for env, pol, roll in rolls:
        roll.close(); pol.close(); env.close()
    per_pass = [(statistics.median(us[0][p]), statistics.median(us[1][p])) for p in (0, 1)]
    pooled = [statistics.median(us[0][p] + us[1][p]) for p in (0, 1)]
    spread = max(abs(x - y) for x, y in per_pass)
    return pooled, per_pass, spread, same, episodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1200, help="timed env steps per path and pass (two passes): steps / K replays")
    ap.add_argument("--warmup", type=int, default=10, help="replays of each path before the timed passes")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if args.steps < 400:
        ap.error("--steps must be at least 400")
    lines = ["the actor loop of crowd worlds with the weight_sharing network, K env steps per hipGraph replay, built as ga3c.train builds it (closest_first, generator in the",
             "step, 2..N agents per world, cleaned re-flush mode, the config's TIME_MAX); HIP events around each replay, the two paths alternating;",
             "us per ENV STEP, medians of 2 passes x %d env steps (%d / K replays) per path (%s)" % (args.steps, args.steps, torch.cuda.get_device_name(0)),
             "fused: capture_fused_crowd_ws(K) = cavoid_crowd_actor_run_ws, one launch per K steps; phases: capture(K) of step() = per step the weight_sharing policy",
             "kernel + cavoid_step_push.  scripted: ga3c.train --scripted-fraction (0.5: static / ORCA / non-cooperative agents, the ORCA-carrying",
             "env step).  spread: the larger |median pass 1 - median pass 2| of the two paths (a repeat of the same path)",
             "",
             "%-6s %-6s %-8s %-3s %-8s | %-27s | %-27s | %-6s | %-12s | %s" % ("agents", "worlds", "observed", "K", "scripted", "fused (pass 1, pass 2)",
                                                                            "phases (pass 1, pass 2)", "spread", "fused/phases", "verdict")]
    for scripted in MIXES:
        for N, W, M in SHAPES:
            for K in KS:
                pooled, per_pass, spread, same, episodes = bench(N, W, M, K, scripted, args.steps // K, args.warmup)
                diff = pooled[0] - pooled[1]
                verdict = "fused slower by more than the spread" if diff > spread else ("fused faster by more than the spread" if -diff > spread
                                                                                        else "within the spread")
                lines.append("%-6d %-6d %-8d %-3d %-8.1f | %7.1f  (%7.1f, %7.1f) | %7.1f  (%7.1f, %7.1f) | %6.1f | %12.3f | %s" % (
                    N, W, M, K, scripted, pooled[0], per_pass[0][0], per_pass[0][1], pooled[1], per_pass[1][0], per_pass[1][1], spread,
                    pooled[0] / pooled[1],
                    verdict + ("; trajectories identical, %d episodes logged" % episodes[0] if same and episodes[0] == episodes[1]
                               else "; TRAJECTORIES DIFFER")))
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
