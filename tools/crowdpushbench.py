#!/usr/bin/env python
"""One `BatchedRollout.step(acts, vals)` on a crowd env (17..64 agents per world), scripted actions, no policy: the ONE launch
(`cavoid_step_push` -> crowd_push_kernel) against the THREE it replaces (crowd_kernel, rollout_push_kernel, rollout_episode_kernel),
in the same process on the same library.

Two twin envs / rollouts (same seed, same actions: their trajectories are bit-identical) take every step one after the other, each step
between two HIP events; the order of the two paths alternates from step to step.  Every shape is warmed up on both paths, then timed
in two passes of `--steps` steps each: the table gives each path's median per pass and over both, and the spread -- the larger of the
two paths' |median of pass 1 - median of pass 2|, what a repeat of the SAME path differs by.  The rule the default follows: the one
launch is the default for crowd envs unless it is slower than the three by more than that spread at some shape
(profiles/crowd_step_push_timing.txt: it is not).

    python tools/crowdpushbench.py [--steps 200] [--out profiles/crowd_step_push_timing.txt]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
from rl_collision_avoidance_amd.config import EnvConfig
from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout

SHAPES = [(20, 2048), (32, 1024), (64, 512)]       # agents per world x worlds: 32 768 rows (40 960 at 20), M = N - 1
PATHS = ("step_push", "env, push, episode log")


def make(N, W, fuse):
    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = N - 1
            EnvConfig.__init__(self)
    env = BatchedCollisionAvoidanceEnv(W, Cfg(), device="cuda:0", seed=3)
    roll = BatchedRollout(env, None, reflush_done=False, time_max=5)
    roll.fuse_env_push = fuse
    roll.reset()
    assert roll.step_path == PATHS[0 if fuse else 1]
    return env, roll


def timed_step(roll, acts, vals):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    roll.step(acts, vals)
    e1.record()
    return e0, e1


def bench_shape(N, W, steps, warmup):
    rolls = [make(N, W, True), make(N, W, False)]
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
    us = []                                                # us[pass][path]: every timed step of that pass
    for _ in range(2):
        events = ([], [])
        for k in range(steps):
            for which in ((0, 1) if k % 2 == 0 else (1, 0)):
                events[which].append(timed_step(rolls[which][1], acts[t % 16], vals[t % 16]))
            t += 1
        torch.cuda.synchronize()
        us.append([[e0.elapsed_time(e1) * 1e3 for e0, e1 in ev] for ev in events])
    same = torch.equal(rolls[0][1].obs, rolls[1][1].obs) and torch.equal(rolls[0][1].emit_t, rolls[1][1].emit_t)
    episodes = [int(r.ep_count[0].item()) for _, r in rolls]
    for env, roll in rolls:
        roll.close(); env.close()
    per_pass = [(statistics.median(us[0][p]), statistics.median(us[1][p])) for p in (0, 1)]
    pooled = [statistics.median(us[0][p] + us[1][p]) for p in (0, 1)]
    spread = max(abs(a - b) for a, b in per_pass)
    return pooled, per_pass, spread, same, episodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="timed steps per path and pass (two passes)")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if args.steps < 200:
        ap.error("--steps must be at least 200")
    lines = ["one BatchedRollout.step(acts, vals) on a crowd env, time_max=5, scripted actions, no policy; HIP events around the step,",
             "the two paths alternating; us, medians of 2 passes x %d steps per path (%s)" % (args.steps, torch.cuda.get_device_name(0)),
             "spread: the larger |median pass 1 - median pass 2| of the two paths (a repeat of the same path)",
             "",
             "%-7s %-7s | %-28s | %-28s | %-7s | %-9s | %s" % ("agents", "worlds", "one launch (pass 1, pass 2)", "three launches (pass 1, 2)", "spread",
                                                              "one/three", "verdict")]
    slower_somewhere = False
    for N, W in SHAPES:
        pooled, per_pass, spread, same, episodes = bench_shape(N, W, args.steps, args.warmup)
        slower = pooled[0] - pooled[1] > spread
        slower_somewhere = slower_somewhere or slower
        lines.append("%-7d %-7d | %7.1f  (%7.1f, %7.1f)  | %7.1f  (%7.1f, %7.1f)  | %7.1f | %9.3f | %s" % (
            N, W, pooled[0], per_pass[0][0], per_pass[0][1], pooled[1], per_pass[1][0], per_pass[1][1], spread, pooled[0] / pooled[1],
            ("one launch slower by more than the spread" if slower else "one launch not slower") +
            ("; trajectories identical, %d episodes logged" % episodes[0] if same and episodes[0] == episodes[1] else "; TRAJECTORIES DIFFER")))
        print(lines[-1], flush=True)
    lines += ["", "what the rule says for crowd envs: %s" % ("the three launches as the default" if slower_somewhere
                                                             else "the one launch (cavoid_step_push) as the default, as for tile envs")]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
