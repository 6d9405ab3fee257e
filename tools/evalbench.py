#!/usr/bin/env python
"""A whole EVALUATE_MODE round of `ga3c.evaluate`: `fused=True` (`cavoid_eval_run` -> eval_kernel: policy, argmax, env step without
auto-reset and the outcome record per tile inside one launch of K env steps, finished tiles leaving early, one 4-byte read per launch)
against `fused=False` (per env step the policy launch, `cavoid_step`, a copy of the world buffer, a handful of mask launches and a host
synchronisation), in the same process on the same library.

One env and one network per shape; every round re-seeds the env, so both paths evaluate the SAME scenarios (their results are compared).
The network is `NetworkVP_rnn` with its initial weights and a bias on action 2 (full speed, straight ahead): rounds with goals and
collisions whose worlds end at widely different steps -- what early exit is about.  The two paths alternate round by round (the order
flips every pair); wall clock around each round with the device synchronised, since the host's part IS what is measured.  Reported per
path: the median of the rounds, the spread (max - min of that path's rounds); then the round's env_steps, the median of world_steps and
the share of tile-steps a fixed-length loop would have spent on finished tiles.

`--arch weight_sharing` measures the weight_sharing network's kernel instead (`fused_ws=True`, `cavoid_eval_run_ws` -> eval_ws_kernel)
against the same step-by-step loop on the weight_sharing handle; `--observed M` sets the observed neighbours of every shape (default: 7 at
4 agents -- WS-8 -- and 9 at 10).

    python tools/evalbench.py [--rounds 5] [--steps-per-launch 16] [--out profiles/eval_fused_timing.txt]
    python tools/evalbench.py --arch weight_sharing [--observed M] [--out profiles/eval_ws_fused_timing.txt]
    rocprofv3 --kernel-trace --stats -- python tools/evalbench.py --only fused --rounds 1      (the kernel's own time)"""
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

SHAPES = [(4, 4096), (10, 1024)]                   # agents per world x worlds
WS_OBSERVED = {4: 7, 10: 9}                        # --arch weight_sharing without --observed: WS-8 at 4 agents, every neighbour at 10
SEED = 3


def make(N, W, arch="rnn", observed=None):
    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            if observed is not None:
                self.MAX_NUM_OTHER_AGENTS_OBSERVED = observed
            EnvConfig.__init__(self)
    cfg = Cfg()
    env = BatchedCollisionAvoidanceEnv(W, cfg, device="cuda:0", seed=SEED, gen_min_agents=2, gen_pool_size=0, evaluate_mode=1)
    net = NetworkVP_rnn(cfg, seed=0, arch=arch).to("cuda:0")
    with torch.no_grad():
        net.p_bias[2] += 1.0
    return env, FusedPolicy(net, seed=77)


def one_round(env, pol, fused, spl):
    env.seed(SEED)                                          # the same scenarios for every round of either path
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = ev.evaluate(env, pol, rounds=1, fused=fused and not pol.ws, fused_ws=fused and pol.ws, steps_per_launch=spl)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def world_steps(env, pol, spl):
    """(not timed) the records of one fused round: every world's step count"""
    env.seed(SEED)
    env.reset()
    rec = ev._EvalRecords(env)
    for _ in range(100000 // spl):
        (ev.eval_run_ws if pol.ws else ev.eval_run)(env, pol, None, rec, spl)
        if int(rec.worlds_running.item()) == 0:
            break
    return rec.world_steps.clone()


def bench(N, W, rounds, spl, only, arch="rnn", observed=None):
    env, pol = make(N, W, arch, observed)
    legs = [leg for leg in (True, False) if only in (None, "fused" if leg else "loop")]
    for leg in legs:                                        # warm-up: one round of each path
        one_round(env, pol, leg, spl)
    ms, res = {True: [], False: []}, {}
    for k in range(rounds):
        for leg in (legs if k % 2 == 0 else legs[::-1]):
            t, res[leg] = one_round(env, pol, leg, spl)
            ms[leg].append(t)
    ws = world_steps(env, pol, spl)
    env_steps = int(ws.max())
    per_tile = 64 // N
    pad = (-W) % per_tile
    tiles = torch.cat([ws, ws.new_zeros(pad)]).view(-1, per_tile).max(dim=1)[0]
    removed = 1.0 - float(tiles.double().mean()) / env_steps
    # (mean_reward apart: the kernel's return stops where the world is over, the loop's goes on summing what cavoid_step pays finished worlds)
    same = len(legs) < 2 or all(res[True][k] == res[False][k] for k in res[True] if k != "mean_reward")
    pol.close(); env.close()
    return ms, env_steps, int(ws.median()), removed, same, res[legs[0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds per path")
    ap.add_argument("--steps-per-launch", type=int, default=16)
    ap.add_argument("--only", default=None, choices=["fused", "loop"], help="run one path only (a profiler run)")
    ap.add_argument("--arch", default="rnn", choices=["rnn", "weight_sharing"], help="the network (weight_sharing: fused_ws=True / cavoid_eval_run_ws)")
    ap.add_argument("--observed", type=int, default=None, metavar="M",
                    help="observed neighbours of every shape (default: agents - 1; with --arch weight_sharing 7 at 4 agents and 9 at 10)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    ws = args.arch == "weight_sharing"
    lines = ["one EVALUATE_MODE round of ga3c.evaluate (env.reset, the whole loop, the reduction), wall clock with the device synchronised, ms per round;",
             "fused: evaluate(%s=True, steps_per_launch=%d) = %s; loop: evaluate(fused=False) = policy launch + cavoid_step + world-buffer"
             % ("fused_ws" if ws else "fused", args.steps_per_launch, "cavoid_eval_run_ws" if ws else "cavoid_eval_run"),
             "copy + mask launches + one host synchronisation per env step.  Same env, seeds and %s network (initial weights, action 2 favoured); the paths"
             % args.arch,
             "alternate; median and spread (max - min) of %d rounds per path (%s)" % (args.rounds, torch.cuda.get_device_name(0)),
             "tile-steps removed: 1 - mean over tiles of the tile's last step / env_steps (what a fixed-length loop spends on finished tiles)",
             "",
             "%-6s %-6s %-8s | %-22s | %-22s | %-10s | %-9s %-18s %-18s | %s" % ("agents", "worlds", "observed", "fused median (spread)", "loop median (spread)", "fused/loop",
                                                                       "env_steps", "median world_steps", "tile-steps removed", "verdict")]
    for N, W in SHAPES:
        M = args.observed if args.observed is not None else (WS_OBSERVED.get(N) if ws else None)
        ms, env_steps, med_ws, removed, same, res = bench(N, W, args.rounds, args.steps_per_launch, args.only, args.arch, M)
        f, l = ms[True], ms[False]
        fm, lm = (statistics.median(f) if f else float("nan")), (statistics.median(l) if l else float("nan"))
        fs, ls = (max(f) - min(f) if f else float("nan")), (max(l) - min(l) if l else float("nan"))
        if f and l:
            verdict = ("fused faster by more than the loop's spread" if lm - fm > ls else
                       "fused slower by more than the loop's spread" if fm - lm > ls else "within the loop's spread")
            verdict += "; results identical (mean_reward apart)" if same else "; RESULTS DIFFER"
        else:
            verdict = "one path only"
        lines.append("%-6d %-6d %-8d | %9.1f (%9.1f) | %9.1f (%9.1f) | %10.3f | %-9d %-18d %-18.3f | %s" % (
            N, W, M if M is not None else N - 1, fm, fs, lm, ls, fm / lm if f and l else float("nan"), env_steps, med_ws, removed, verdict))
        lines.append("       success %.4f collision %.4f timeout %.4f over %d learning agents" % (
            res["success_rate"], res["collision_rate"], res["timeout_rate"], res["agents"]))
        print(lines[-2], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
