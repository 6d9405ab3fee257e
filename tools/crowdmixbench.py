#!/usr/bin/env python
"""Crowd worlds (17..64 agents per world) with FROZEN-NETWORK agents, the published training mix (`ga3c.train --agents N --scripted-fraction
S --frozen-fraction F`): the two launches that carry the second network against the paths of before, in the same process on the same
library.

Actors: K env steps per hipGraph replay -- the ONE launch of `capture_fused_crowd_mix(K)` (`cavoid_crowd_actor_run_mix` ->
crowd_mix_rollout_kernel: policy pass, the pass once more on the frozen network where a tile holds a running frozen-network agent, action
draw, env step, Experience bookkeeping per tile inside one kernel) against `capture(K)` of `step()` with the same `frozen_policy` (per env
step the crowd policy kernel, `cavoid_policy_rows`, the frozen network's row-list launch, `cavoid_step_push`).  Twin rollouts of the same
seeds replay their graphs one after the other, each replay between two HIP events, the order alternating; tools/crowdactorbench.py's
scheme: two passes, the medians per pass and over both in us per ENV STEP, and the spread (what a repeat of the SAME path differs by).

Evaluation: one whole EVALUATE_MODE round by wall clock with the device synchronised -- `evaluate(fused_crowd_mix=True,
steps_per_launch=K)` (`cavoid_crowd_eval_run_mix`) against the step-by-step `evaluate(frozen_policy=...)`; tools/crowdevalbench.py's
scheme: the two paths alternate, `--rounds` rounds each in two passes.

    python tools/crowdmixbench.py [--scripted-fraction 0.5] [--frozen-fraction 0.5] [--steps 1200] [--rounds 3] [--out profiles/crowd_mix_timing.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
from rl_collision_avoidance_amd.config import EnvConfig
from rl_collision_avoidance_amd.ga3c import evaluate as ev
from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout

SHAPES = [(20, 2048), (32, 1024), (64, 512)]       # agents per world x worlds: 32 768 rows (40 960 at 20), M = N - 1
KS = (4, 16)                                       # env steps per replay: ga3c.train's default, and a long launch
EVAL_K = 16


def config(N, scripted, frozen):
    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            self.SCRIPTED_AGENT_FRACTION = scripted
            self.SCRIPTED_STATIC_FRACTION = 0.34
            self.SCRIPTED_RVO_FRACTION = 0.33 if scripted > 0 else 0.0
            self.SCRIPTED_FROZEN_NET_FRACTION = frozen if scripted > 0 else 0.0
            EnvConfig.__init__(self)
    return Cfg()


def policies(cfg):
    torch.manual_seed(1234)
    pol = FusedPolicy(NetworkVP_rnn(cfg, seed=0).to("cuda:0"), seed=77)
    fz = FusedPolicy(NetworkVP_rnn(cfg, seed=4321).to("cuda:0"), seed=0)
    return pol, fz


def make_actor(N, W, K, scripted, frozen, fused):
    cfg = config(N, scripted, frozen)
    env = BatchedCollisionAvoidanceEnv(W, cfg, device="cuda:0", seed=3, gen_min_agents=2, gen_pool_size=0)
    pol, fz = policies(cfg)
    time_max = int(getattr(cfg, "TIME_MAX", int(4 / cfg.DT)))
    roll = BatchedRollout(env, pol, reflush_done=False, ring_len=max(time_max + 2 + K + 8, 2 * (time_max + 2) + 8), frozen_policy=fz)
    roll.reset()
    if fused:
        assert roll.crowd_mix_fused_available, roll.crowd_mix_fused_unavailable_reason
        roll.capture_fused_crowd_mix(K)
    else:
        assert not roll.fused_available
        roll.capture(K)
    return env, (pol, fz), roll


def timed_replay(roll):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    roll.replay(1)
    e1.record()
    return e0, e1


def bench_actor(N, W, K, scripted, frozen, replays, warmup):
    rolls = [make_actor(N, W, K, scripted, frozen, True), make_actor(N, W, K, scripted, frozen, False)]
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
        us.append([[e0.elapsed_time(e1) * 1e3 / K for e0, e1 in evs] for evs in events])
    (ea, _, a), (eb, _, b) = rolls
    # (the value / action rings of rows that need no action are never read and differ by design, as in tools/crowdactorbench.py)
    same = (torch.equal(a.obs, b.obs) and torch.equal(a.emit_t, b.emit_t) and torch.equal(a.x, b.x) and torch.equal(a.ret, b.ret)
            and all(torch.equal(u, v) for u, v in zip(ea.get_state(), eb.get_state())))
    episodes = [int(r.ep_count[0].item()) for _, _, r in rolls]
    form = ea.last_step_form[0]
    for env, (pol, fz), roll in rolls:
        roll.close(); pol.close(); fz.close(); env.close()
    per_pass = [(statistics.median(us[0][p]), statistics.median(us[1][p])) for p in (0, 1)]
    pooled = [statistics.median(us[0][p] + us[1][p]) for p in (0, 1)]
    spread = max(abs(x - y) for x, y in per_pass)
    return pooled, per_pass, spread, same, episodes, form


def one_round(env, pol, fz, fused, spl, max_steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ev.evaluate(env, pol, rounds=1, frozen_policy=fz, fused_crowd_mix=fused, steps_per_launch=spl, max_steps=max_steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def bench_eval(N, W, scripted, frozen, rounds, max_steps):
    cfg = config(N, scripted, frozen)
    envs = [BatchedCollisionAvoidanceEnv(W, cfg, device="cuda:0", seed=3, gen_min_agents=2, gen_pool_size=0, evaluate_mode=1) for _ in range(2)]
    pols = [policies(cfg) for _ in range(2)]
    assert ev.evaluate_fused_crowd_mix_unavailable_reason(envs[0], *pols[0]) is None
    for which in (0, 1):                                   # one warm-up round of each path
        one_round(envs[which], *pols[which], which == 0, EVAL_K, max_steps)
    ms, results = [], [None, None]
    for _ in range(2):
        t = ([], [])
        for k in range(rounds):
            for which in ((0, 1) if k % 2 == 0 else (1, 0)):
                dt, results[which] = one_round(envs[which], *pols[which], which == 0, EVAL_K, max_steps)
                t[which].append(dt)
        ms.append(t)
    # (every round resets the env from its own seed stream: the two envs run the same rounds in the same order)
    same = all(results[0][k] == results[1][k] for k in results[0] if k != "mean_reward")
    steps = results[0]["env_steps"]
    for env, (pol, fz) in zip(envs, pols):
        pol.close(); fz.close(); env.close()
    per_pass = [(statistics.median(ms[0][p]), statistics.median(ms[1][p])) for p in (0, 1)]
    pooled = [statistics.median(ms[0][p] + ms[1][p]) for p in (0, 1)]
    spread = max(abs(x - y) for x, y in per_pass)
    return pooled, per_pass, spread, same, steps


def verdict(diff, spread):
    return "fused slower by more than the spread" if diff > spread else ("fused faster by more than the spread" if -diff > spread else "within the spread")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scripted-fraction", type=float, default=0.5, help="ga3c.train --scripted-fraction")
    ap.add_argument("--frozen-fraction", type=float, default=0.5, help="ga3c.train --frozen-fraction (of the scripted agents)")
    ap.add_argument("--steps", type=int, default=1200, help="actors: timed env steps per path and pass (two passes): steps / K replays")
    ap.add_argument("--warmup", type=int, default=10, help="actors: replays of each path before the timed passes")
    ap.add_argument("--rounds", type=int, default=3, help="evaluation: timed rounds per path and pass (two passes)")
    ap.add_argument("--max-steps", type=int, default=400, help="evaluation: the cut of a round, in env steps")
    ap.add_argument("--skip-actors", action="store_true")
    ap.add_argument("--skip-evaluation", action="store_true")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    if args.steps < 400:
        ap.error("--steps must be at least 400")
    S, F = args.scripted_fraction, args.frozen_fraction
    lines = ["crowd worlds with frozen-network agents (--scripted-fraction %.2f --frozen-fraction %.2f; ga3c.train's --static-fraction / --rvo-fraction:" % (S, F),
             "the ORCA-carrying env step), built as ga3c.train builds them (generator in the step, 2..N agents per world) (%s)" % torch.cuda.get_device_name(0),
             "spread: the larger |median pass 1 - median pass 2| of the two paths (a repeat of the same path)", ""]
    if not args.skip_actors:
        lines += ["ACTORS, K env steps per hipGraph replay; HIP events around each replay, the two paths alternating; us per ENV STEP, medians of",
                  "2 passes x %d env steps per path.  fused: capture_fused_crowd_mix(K) = cavoid_crowd_actor_run_mix, one launch per K steps; phases:" % args.steps,
                  "capture(K) of step() with the same frozen_policy", "",
                  "%-6s %-6s %-3s %-9s | %-27s | %-27s | %-6s | %-12s | %s" % ("agents", "worlds", "K", "env step", "fused (pass 1, pass 2)",
                                                                           "phases (pass 1, pass 2)", "spread", "fused/phases", "verdict")]
        for N, W in SHAPES:
            for K in KS:
                pooled, per_pass, spread, same, episodes, form = bench_actor(N, W, K, S, F, args.steps // K, args.warmup)
                lines.append("%-6d %-6d %-3d %-9s | %7.1f  (%7.1f, %7.1f) | %7.1f  (%7.1f, %7.1f) | %6.1f | %12.3f | %s" % (
                    N, W, K, form, pooled[0], per_pass[0][0], per_pass[0][1], pooled[1], per_pass[1][0], per_pass[1][1], spread, pooled[0] / pooled[1],
                    verdict(pooled[0] - pooled[1], spread) + ("; trajectories identical, %d episodes logged" % episodes[0]
                                                              if same and episodes[0] == episodes[1] else "; TRAJECTORIES DIFFER")))
                print(lines[-1], flush=True)
        lines.append("")
    if not args.skip_evaluation:
        lines += ["EVALUATION, one whole round (cut at %d env steps) by wall clock with the device synchronised, ms per round, medians of 2 passes x %d" % (
                      args.max_steps, args.rounds),
                  "rounds per path, the two paths alternating.  fused: evaluate(fused_crowd_mix=True, steps_per_launch=%d) = cavoid_crowd_eval_run_mix;" % EVAL_K,
                  "loop: evaluate(frozen_policy=...) = policy launch + cavoid_policy_rows + frozen network's launch + cavoid_step + one host",
                  "synchronisation per env step", "",
                  "%-6s %-6s %-9s | %-27s | %-27s | %-6s | %-10s | %s" % ("agents", "worlds", "env steps", "fused (pass 1, pass 2)", "loop (pass 1, pass 2)",
                                                                      "spread", "fused/loop", "verdict")]
        for N, W in SHAPES:
            pooled, per_pass, spread, same, steps = bench_eval(N, W, S, F, args.rounds, args.max_steps)
            lines.append("%-6d %-6d %-9d | %7.1f  (%7.1f, %7.1f) | %7.1f  (%7.1f, %7.1f) | %6.1f | %10.3f | %s" % (
                N, W, steps, pooled[0], per_pass[0][0], per_pass[0][1], pooled[1], per_pass[1][0], per_pass[1][1], spread, pooled[0] / pooled[1],
                verdict(pooled[0] - pooled[1], spread) + ("; same statistics" if same else "; STATISTICS DIFFER")))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
