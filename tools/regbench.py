"""Time one step of the supervised start on the fused trainer kernels against the PyTorch autograd step ``regression.pretrain`` runs
without a trainer (development aid).
usage: python tools/regbench.py [rows] [--reps 40] [--rounds 3] [--pretrain-steps 300]
For rnn M = 3 and weight_sharing M = 7: per round, the median of --reps HIP-event-timed steps after 5 warm-up steps, alternating
  fused:    FusedA3CTrainer.train_regression (launch pair, weight-gradient GEMMs, Adam step, weight re-pack)
  autograd: regression_loss + backward + Adam.step, with the two host reads of the losses pretrain makes per step
(Adam(lr=0, eps=1e-8) on both sides: the weights stay put).  Then the wall time of pretrain(steps=--pretrain-steps) on each path,
teacher rollouts included (4-agent worlds: rnn and weight_sharing M = 3)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
from rl_collision_avoidance_amd.config import EnvConfig
from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
from rl_collision_avoidance_amd.ga3c.regression import pretrain, regression_loss


def median_us(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rows", type=int, nargs="?", default=32768)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pretrain-steps", type=int, default=300)
    args = ap.parse_args()
    B = args.rows
    print("arch            M  rows    fused step (us)          autograd step (us)")
    for arch, M in (("rnn", 3), ("weight_sharing", 7)):
        class Cfg(EnvConfig):
            def __init__(self):
                self.MAX_NUM_AGENTS_IN_ENVIRONMENT = M + 1
                EnvConfig.__init__(self)
        net = NetworkVP_rnn(Cfg(), arch=arch).cuda()
        g = torch.Generator().manual_seed(0)
        x = torch.randn((B, net.input_size), generator=g) * net.std.cpu() + net.avg.cpu()
        x[:, 0] = torch.randint(0, M + 1, (B,), generator=g).float()
        x, y, a = x.cuda(), torch.randn(B, generator=g).cuda(), torch.randint(0, net.num_actions, (B,), generator=g).cuda()
        opt = torch.optim.Adam(net.parameters(), lr=0.0, eps=1e-8)
        tr = FusedA3CTrainer(net, learning_rate=0.0)

        def fused():
            tr.train_regression(x, y, a, opt=opt)

        def autograd():
            opt.zero_grad(set_to_none=True)
            total, cost_p, cost_v = regression_loss(net, x, y, a)
            total.backward()
            opt.step()
            return float(cost_p.detach()) / B, float(cost_v.detach()) / B
        t_f, t_a = [], []
        for _ in range(args.rounds):
            t_f.append(median_us(fused, args.reps))
            t_a.append(median_us(autograd, args.reps))
        print("%-15s %-2d %-7d %-24s %-24s %.2fx" % (arch, M, B, " ".join("%.1f" % t for t in t_f), " ".join("%.1f" % t for t in t_a),
                                                      statistics.median(t_a) / statistics.median(t_f)), flush=True)
    if args.pretrain_steps <= 0:
        return
    print("pretrain(steps=%d, rows_per_step=%d), 8192 worlds of 4 agents, wall time in s (teacher rollouts included)" % (args.pretrain_steps, B))
    for arch in ("rnn", "weight_sharing"):
        for path in ("fused", "autograd"):
            env = BatchedCollisionAvoidanceEnv(8192, seed=1)
            net = NetworkVP_rnn(env.config, arch=arch).cuda()
            tr = FusedA3CTrainer(net) if path == "fused" else None
            torch.cuda.synchronize()
            t0 = time.time()
            info = pretrain(net, env, steps=args.pretrain_steps, rows_per_step=B, trainer=tr)
            torch.cuda.synchronize()
            print("%-15s %-9s %.2f s   p-loss/row %.4f  v-loss/row %.5f" % (arch, path, time.time() - t0, info["p_loss_per_row"],
                                                                         info["v_loss_per_row"]), flush=True)
            env.close()


if __name__ == "__main__":
    main()
