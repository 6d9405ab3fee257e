#!/usr/bin/env python
"""What ORCA agents cost a crowd env (17..64 agents per world): one `BatchedRollout.step(acts, vals)` -- `cavoid_step_push`, scripted
actions, no policy -- on worlds whose scripted agents are

    none    --scripted-fraction 0.5 --rvo-fraction 0     no ORCA agent: crowd_push_kernel, the kernel of before (the baseline)
    mix     --scripted-fraction 0.5 --rvo-fraction 0.33  ga3c.train's default mix: crowd_rvo_push_kernel
    worst   --scripted-fraction 0.9 --rvo-fraction 1.0   nearly every agent an ORCA agent

at 20 x 2048, 32 x 1024 and 64 x 512, in one process on one library.  The envs of a shape take every step one after the other, each
step between two HIP events, the order rotating from step to step.  Every shape is warmed up, then timed in two passes of `--steps`
steps: the table gives each configuration's median per pass and over both, its ratio to `none`, and the spread -- the largest
|median of pass 1 - median of pass 2| of the configurations, what a repeat of the same measurement differs by.  The scenarios are boxes
generated inside the step (ga3c.train's), so the share of running ORCA agents is that of a training run in its steady state; it is
printed per configuration.

`--configs none` with CAVOID_LIB=<a library of the parent commit> gives the baseline on that build (crowd_push_kernel's instruction
stream is the same in both, so the two `none` rows agree to the spread).

    python tools/crowdrvobench.py [--steps 200] [--configs none,mix,worst] [--out profiles/crowd_rvo_timing.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
from rl_collision_avoidance_amd.config import EnvConfig
from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout

SHAPES = [(20, 2048), (32, 1024), (64, 512)]       # agents per world x worlds, M = N - 1
CONFIGS = {"none": (0.5, 0.0), "mix": (0.5, 0.33), "worst": (0.9, 1.0)}     # (scripted fraction, P(ORCA | scripted))
STATIC = 0.34                                      # ga3c.train's --static-fraction


def make(N, W, scripted, rvo):
    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = N - 1
            self.TEST_CASE_GENERATOR = "box"
            self.SCRIPTED_AGENT_FRACTION = scripted
            self.SCRIPTED_STATIC_FRACTION = STATIC if rvo < 1.0 else 0.0
            self.SCRIPTED_RVO_FRACTION = rvo
            EnvConfig.__init__(self)
    env = BatchedCollisionAvoidanceEnv(W, Cfg(), device="cuda:0", seed=3, gen_min_agents=2, gen_pool_size=0)
    roll = BatchedRollout(env, None, reflush_done=False, time_max=5)
    roll.reset()
    assert roll.step_path == "step_push"
    return env, roll


def running_orca_share(env):
    flags = env.get_state()[2].view(torch.int32)
    present = (flags & 0x20) != 0
    orca = present & (((flags >> 8) & 7) == 3) & ((flags & 7) == 0)
    return float(orca.sum().item()) / max(1, int(present.sum().item()))


def bench_shape(N, W, names, steps, warmup):
    rolls = [make(N, W, *CONFIGS[name]) for name in names]
    g = torch.Generator(device="cuda").manual_seed(5)
    acts = torch.randint(0, 11, (16, W, N), generator=g, device="cuda", dtype=torch.int32)
    acts[torch.rand((16, W, N), generator=g, device="cuda") < 0.8] = 2          # mostly 'full speed straight ahead': goals are reached, worlds restart
    vals = torch.randn((16, W, N), generator=g, device="cuda")
    t = 0
    for _ in range(warmup):
        for _, roll in rolls:
            roll.step(acts[t % 16], vals[t % 16])
        t += 1
    torch.cuda.synchronize()
    us, share = [], [0.0] * len(names)
    for _ in range(2):
        events = [[] for _ in names]
        for k in range(steps):
            for j in range(len(names)):
                which = (j + k) % len(names)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rolls[which][1].step(acts[t % 16], vals[t % 16])
                e1.record()
                events[which].append((e0, e1))
            t += 1
        torch.cuda.synchronize()
        us.append([[e0.elapsed_time(e1) * 1e3 for e0, e1 in ev] for ev in events])
        for j, (env, _) in enumerate(rolls):
            share[j] += 0.5 * running_orca_share(env)
    forms = [env.last_step_form[0] for env, _ in rolls]
    episodes = [int(roll.ep_count[0].item()) for _, roll in rolls]
    for env, roll in rolls:
        roll.close(); env.close()
    per_pass = [(statistics.median(us[0][j]), statistics.median(us[1][j])) for j in range(len(names))]
    pooled = [statistics.median(us[0][j] + us[1][j]) for j in range(len(names))]
    return pooled, per_pass, max(abs(a - b) for a, b in per_pass), share, forms, episodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="timed steps per configuration and pass (two passes)")
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--configs", default="none,mix,worst")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    names = [n for n in args.configs.split(",") if n]
    if any(n not in CONFIGS for n in names) or not names:
        ap.error("--configs: a comma-separated list of %s" % ", ".join(CONFIGS))
    if args.steps < 200:
        ap.error("--steps must be at least 200")
    lines = ["one BatchedRollout.step(acts, vals) (cavoid_step_push) on a crowd env, box scenarios generated in the step, time_max=5, scripted actions,",
             "no policy; HIP events around the step, the configurations taking turns; us, medians of 2 passes x %d steps (%s)" % (args.steps, torch.cuda.get_device_name(0)),
             "library: %s" % os.environ.get("CAVOID_LIB", "the in-tree build"),
             "spread: the largest |median pass 1 - median pass 2| of the shape's configurations (a repeat of the same measurement)",
             "running ORCA: the share of the present agents that are ORCA agents still running, mean of the state after each pass",
             "",
             "%-7s %-7s %-6s %-10s | %-28s | %-7s | %-8s | %-12s | %s" % ("agents", "worlds", "config", "form", "us (pass 1, pass 2)", "spread", "/ none", "running ORCA", "episodes")]
    for N, W in SHAPES:
        pooled, per_pass, spread, share, forms, episodes = bench_shape(N, W, names, args.steps, args.warmup)
        base = pooled[names.index("none")] if "none" in names else None
        for j, name in enumerate(names):
            lines.append("%-7d %-7d %-6s %-10s | %7.1f  (%7.1f, %7.1f)  | %7.1f | %-8s | %11.1f%% | %d" % (
                N, W, name, forms[j], pooled[j], per_pass[j][0], per_pass[j][1], spread, "%.2f" % (pooled[j] / base) if base else "-",
                100.0 * share[j], episodes[j]))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
