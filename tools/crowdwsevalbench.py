#!/usr/bin/env python
"""A whole EVALUATE_MODE round of `ga3c.evaluate` on CROWD worlds (17 to 64 agents per world) with the weight_sharing network:
`fused_crowd_ws=True` (`cavoid_crowd_eval_run_ws` -> crowd_ws_evaluate_kernel: the ring form of the weight_sharing pass on the tile's rows
that still need an action, argmax, the crowd env step without auto-reset and the outcome record per tile inside one launch of K env steps,
finished tiles leaving early, one 4-byte read per launch) against the step-by-step round (per env step the weight_sharing policy launch --
the ring kernel above 19 observed neighbours --, `cavoid_step`, a copy of the world buffer, a handful of mask launches and a host
synchronisation), in the same process on the same library.  tools/crowdevalbench.py for the weight_sharing network; the step-by-step leg
is code the kernel does not touch.

One env and one network per row; every round re-seeds the env, so both paths evaluate the SAME scenarios (their results are compared).
The shapes are tools/crowdwsactorbench.py's: WS-8 (`--observed 7 --sort-method closest_first`) in 20-agent worlds, and every neighbour
observed on the ring handle at 32 and 64 agents per world; `--scripted-fraction F` adds the first shape with that share of scripted
agents (ga3c.train's default static / ORCA shares: the ORCA-carrying env step).  The network is `NetworkVP_rnn(arch="weight_sharing")` with
its initial weights and a bias on action 2 (full speed, straight ahead).  The two paths alternate round by round (the order flips every
pair); wall clock around each round with the device synchronised, since the host's part IS what is measured.  Reported per path: the
median of the rounds and the spread (max - min of that path's rounds: how much repeats of the same path differ); then the round's
env_steps, the median of world_steps and the share of tile-steps that early exit removed.

    python tools/crowdwsevalbench.py [--rounds 5] [--steps-per-launch 16] [--scripted-fraction 0.5] [--out profiles/crowd_ws_eval_fused_timing.txt]
    rocprofv3 --kernel-trace --stats -- python tools/crowdwsevalbench.py --only fused --rounds 1      (the kernel's own time)"""
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
from rl_collision_avoidance_amd.ga3c.policy_kernel import MAX_OTHERS_WS, FusedPolicy

SHAPES = [(20, 2048, 7), (32, 1024, 31), (64, 512, 63)]       # agents per world x worlds x observed neighbours
SEED = 3


def make(N, W, M, scripted):
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
    env = BatchedCollisionAvoidanceEnv(W, cfg, device="cuda:0", seed=SEED, gen_min_agents=2, evaluate_mode=1)
    net = NetworkVP_rnn(cfg, seed=0, arch="weight_sharing").to("cuda:0")
    with torch.no_grad():
        net.p_bias[2] += 1.0
    return env, FusedPolicy(net, seed=77, ws_crowd=M > MAX_OTHERS_WS)


def one_round(env, pol, fused, spl, max_steps):
    env.seed(SEED)                                          # the same scenarios for every round of either path
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ev.evaluate(env, pol, rounds=1, fused_crowd_ws=fused, steps_per_launch=spl, max_steps=max_steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def world_steps(env, pol, spl, max_steps):
    """(not timed) the records of one fused round: every world's step count, and the launches the round took"""
    env.seed(SEED)
    env.reset()
    rec = ev._EvalRecords(env)
    launches, steps = 0, 0
    while steps < max_steps:
        n = min(spl, max_steps - steps)
        ev.eval_run_crowd_ws(env, pol, None, rec, n)
        launches += 1
        steps += n
        if int(rec.worlds_running.item()) == 0:
            break
    return rec.world_steps.clone(), launches


def bench(N, W, M, scripted, rounds, spl, only, max_steps):
    env, pol = make(N, W, M, scripted)
    why = ev.evaluate_fused_crowd_ws_unavailable_reason(env, pol)
    if why is not None:
        raise SystemExit("%d x %d, M = %d: the crowd weight_sharing evaluation kernel does not apply: %s" % (N, W, M, why))
    legs = [leg for leg in (True, False) if only in (None, "fused" if leg else "loop")]
    for leg in legs:                                        # warm-up: one round of each path
        one_round(env, pol, leg, spl, max_steps)
    ms, res = {True: [], False: []}, {}
    for k in range(rounds):
        for leg in (legs if k % 2 == 0 else legs[::-1]):
            t, res[leg] = one_round(env, pol, leg, spl, max_steps)
            ms[leg].append(t)
    ws, launches = world_steps(env, pol, spl, max_steps)
    env_steps = int(ws.max())
    per_tile = 64 // N
    pad = (-W) % per_tile
    tiles = torch.cat([ws, ws.new_zeros(pad)]).view(-1, per_tile).max(dim=1)[0]
    removed = 1.0 - float(tiles.double().mean()) / env_steps
    # (mean_reward apart: the kernel's return stops where the world is over, the loop's goes on summing what cavoid_step pays finished worlds)
    same = len(legs) < 2 or all(res[True][k] == res[False][k] for k in res[True] if k != "mean_reward")
    pol.close(); env.close()
    return ms, env_steps, int(ws.median()), removed, same, res[legs[0]], launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds per path")
    ap.add_argument("--steps-per-launch", type=int, default=16)
    ap.add_argument("--scripted-fraction", type=float, default=0.0, help="> 0: one more row, the first shape with this share of scripted agents")
    ap.add_argument("--max-steps", type=int, default=100000, help="cut every round of either path at this many env steps (evaluate's max_steps)")
    ap.add_argument("--only", default=None, choices=["fused", "loop"], help="run one path only (a profiler run)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    lines = ["one EVALUATE_MODE round of ga3c.evaluate on crowd worlds with the weight_sharing network (env.reset, the whole loop, the reduction), wall",
             "clock with the device synchronised, ms per round; fused: evaluate(fused_crowd_ws=True, steps_per_launch=%d) = cavoid_crowd_eval_run_ws; loop:"
             % args.steps_per_launch,
             "evaluate() = weight_sharing policy launch + cavoid_step + world-buffer copy + mask launches + one host synchronisation per env step.  Same",
             "env, seeds and network (initial weights, action 2 favoured, closest_first); the paths alternate; median and spread (max - min: what repeats",
             "of the same path differ by) of %d rounds per path (%s)" % (args.rounds, torch.cuda.get_device_name(0)),
             "tile-steps removed: 1 - mean over tiles of the tile's last step / env_steps (what a fixed-length loop spends on finished tiles)",
             "",
             "%-6s %-6s %-3s %-8s | %-22s | %-22s | %-10s | %-9s %-18s %-18s %-8s | %s" % (
                 "agents", "worlds", "M", "scripted", "fused median (spread)", "loop median (spread)", "fused/loop", "env_steps", "median world_steps",
                 "tile-steps removed", "launches", "verdict")]
    rows = [(N, W, M, 0.0) for N, W, M in SHAPES]
    if args.scripted_fraction > 0.0:
        rows.append(SHAPES[0] + (args.scripted_fraction,))
    for N, W, M, scripted in rows:
        ms, env_steps, med_ws, removed, same, res, launches = bench(N, W, M, scripted, args.rounds, args.steps_per_launch, args.only, args.max_steps)
        f, l = ms[True], ms[False]
        fm, lm = (statistics.median(f) if f else float("nan")), (statistics.median(l) if l else float("nan"))
        fs, ls = (max(f) - min(f) if f else float("nan")), (max(l) - min(l) if l else float("nan"))
        if f and l:
            verdict = ("fused faster by more than the loop's spread" if lm - fm > ls else
                       "FUSED SLOWER by more than the loop's spread" if fm - lm > ls else "within the loop's spread")
            verdict += "; results identical (mean_reward apart)" if same else "; RESULTS DIFFER"
        else:
            verdict = "one path only"
        lines.append("%-6d %-6d %-3d %-8.2f | %9.1f (%9.1f) | %9.1f (%9.1f) | %10.3f | %-9d %-18d %-18.3f %-8d | %s" % (
            N, W, M, scripted, fm, fs, lm, ls, fm / lm if f and l else float("nan"), env_steps, med_ws, removed, launches, verdict))
        lines.append("       success %.4f collision %.4f timeout %.4f unfinished %.4f over %d learning agents; rounds fused %s loop %s" % (
            res["success_rate"], res["collision_rate"], res["timeout_rate"], res["unfinished_rate"], res["agents"],
            " ".join("%.1f" % t for t in f), " ".join("%.1f" % t for t in l)))
        print(lines[-2], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
