"""Time one trainer step of the fused trainer against the autograd trainer on the same rows, up to crowd rows (development aid).
usage: python tools/trainbench.py [rows] [max_other ...] [--reps 10] [--rounds 3] [--arch rnn|weight_sharing]
For each max_other (default 19 31 63) at `rows` rows (default 16384): per round, the median of --reps HIP-event-timed steps after 5
warm-up steps, alternating
  fused:    FusedA3CTrainer.train (launch pair -- above 19 observed neighbours the ring forward kernel, crowd=True -- weight-gradient GEMMs,
            Adam step, weight re-pack)
  autograd: A3CTrainer.train (NetworkVP_rnn.loss + backward + Adam step)
(learning rate 0 on both sides: the weights stay put).  Row lengths are drawn uniformly from 0 .. max_other.  The fused trainer's scratch is
printed with each line (FusedA3CTrainer.scratch_bytes).  Figures go to profiles/policy_crowd_train_timing.txt.
--arch weight_sharing: the same for the weight-sharing network -- above 19 observed neighbours the ring forward kernel of
cavoid_policy_wsring.hpp, ws_crowd=True; figures go to profiles/policy_wsring_timing.txt.
--device-step: another pair of legs ('rnn' only; `rows` and `max_other` are ignored: 32 768 rows at M = 3, 16 384 rows at M = 19 and 63) --
  torch tail:   FusedA3CTrainer.train as above (library GEMMs, index_selects, torch.optim.Adam, re-pack)
  device step:  FusedA3CTrainer(device_step=True).train (cavoid_policy_weight_grads + cavoid_policy_apply behind the same launch pair)
alternating on the same rows, and the two new calls timed apart on the buffers of the last step.  Per leg: the rounds' medians, their
median and their spread (max - min over the rounds); figures go to profiles/policy_device_step_timing.txt.
--ws-device-step: the same two legs for the weight-sharing network (32 768 rows at M = 7, 16 384 rows at M = 19 and at M = 63, ws_crowd) --
FusedA3CTrainer.train against FusedA3CTrainer(ws_device_step=True).train (cavoid_policy_weight_grads_ws + cavoid_policy_apply_ws), and the two
new calls apart; figures go to profiles/policy_ws_device_step_timing.txt."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rl_collision_avoidance_amd.config import EnvConfig
from rl_collision_avoidance_amd.ga3c.network import A3CTrainer, NetworkVP_rnn
from rl_collision_avoidance_amd.ga3c.policy_kernel import MAX_OTHERS, MAX_OTHERS_WS, FusedA3CTrainer


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


def device_step_legs(reps, rounds, ws=False):
    print("M   rows    torch tail step (us)           device step (us)               weight_grads%s (us)     apply%s (us)            torch / device"
          % (("_ws", "_ws") if ws else ("", "")))
    for M, B in ((7 if ws else 3, 32768), (19, 16384), (63, 16384)):
        class Cfg(EnvConfig):
            def __init__(self):
                self.MAX_NUM_AGENTS_IN_ENVIRONMENT = M + 1
                EnvConfig.__init__(self)
        arch = "weight_sharing" if ws else "rnn"
        net_t, net_d = NetworkVP_rnn(Cfg(), arch=arch).cuda(), NetworkVP_rnn(Cfg(), arch=arch).cuda()
        g = torch.Generator().manual_seed(0)
        x = torch.randn((B, net_t.input_size), generator=g) * net_t.std.cpu() + net_t.avg.cpu()
        x[:, 0] = torch.randint(0, M + 1, (B,), generator=g).float()
        x, y, a = x.cuda(), torch.randn(B, generator=g).cuda(), torch.randint(0, net_t.num_actions, (B,), generator=g).cuda()
        if ws:
            tt = FusedA3CTrainer(net_t, learning_rate=0.0, ws_crowd=M > MAX_OTHERS_WS)
            td = FusedA3CTrainer(net_d, learning_rate=0.0, ws_crowd=M > MAX_OTHERS_WS, ws_device_step=True)
        else:
            tt = FusedA3CTrainer(net_t, learning_rate=0.0, crowd=M > MAX_OTHERS)
            td = FusedA3CTrainer(net_d, learning_rate=0.0, crowd=M > MAX_OTHERS, device_step=True)
        rows64 = FusedA3CTrainer.buffer_rows(B)
        t_t, t_d, t_g, t_a = [], [], [], []
        for _ in range(rounds):
            t_t.append(median_us(lambda: tt.train(x, y, a), reps))
            t_d.append(median_us(lambda: td.train(x, y, a), reps))
            bufs, cbuf = td._scratch(rows64)                     # (filled by the step just timed)
            t_g.append(median_us(lambda: td._weight_grads(bufs, cbuf, rows64), reps))
            t_a.append(median_us(td._apply, reps))
        cell = lambda t: "%s | %.0f +- %.0f" % (" ".join("%.0f" % v for v in t), statistics.median(t), max(t) - min(t))
        print("%-3d %-7d %-30s %-30s %-21s %-21s %.2fx" % (M, B, cell(t_t), cell(t_d), cell(t_g), cell(t_a),
                                                             statistics.median(t_t) / statistics.median(t_d)), flush=True)
        del tt, td, net_t, net_d
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rows", type=int, nargs="?", default=16384)
    ap.add_argument("max_other", type=int, nargs="*", default=[19, 31, 63])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--arch", default="rnn", choices=["rnn", "weight_sharing"])
    ap.add_argument("--device-step", action="store_true")
    ap.add_argument("--ws-device-step", action="store_true")
    args = ap.parse_args()
    if args.device_step or args.ws_device_step:
        return device_step_legs(args.reps, args.rounds, ws=args.ws_device_step)
    B = args.rows
    print("M   rows    scratch (GB)  fused step (us)                autograd step (us)             autograd / fused")
    for M in args.max_other:
        class Cfg(EnvConfig):
            def __init__(self):
                self.MAX_NUM_AGENTS_IN_ENVIRONMENT = M + 1
                EnvConfig.__init__(self)
        net_f = NetworkVP_rnn(Cfg(), arch=args.arch).cuda()
        net_a = NetworkVP_rnn(Cfg(), arch=args.arch).cuda()
        g = torch.Generator().manual_seed(0)
        x = torch.randn((B, net_f.input_size), generator=g) * net_f.std.cpu() + net_f.avg.cpu()
        x[:, 0] = torch.randint(0, M + 1, (B,), generator=g).float()
        x, y, a = x.cuda(), torch.randn(B, generator=g).cuda(), torch.randint(0, net_f.num_actions, (B,), generator=g).cuda()
        onehot = torch.nn.functional.one_hot(a, net_f.num_actions).float()
        if args.arch == "weight_sharing":
            tf = FusedA3CTrainer(net_f, learning_rate=0.0, ws_crowd=M > MAX_OTHERS_WS)
        else:
            tf = FusedA3CTrainer(net_f, learning_rate=0.0, crowd=M > MAX_OTHERS)
        ta = A3CTrainer(net_a, learning_rate=0.0)
        t_f, t_a = [], []
        for _ in range(args.rounds):
            t_f.append(median_us(lambda: tf.train(x, y, a), args.reps))
            t_a.append(median_us(lambda: ta.train(x, y, onehot), args.reps))
        print("%-3d %-7d %-13.2f %-30s %-30s %.2fx" % (M, B, FusedA3CTrainer.scratch_bytes(M, FusedA3CTrainer.buffer_rows(B), arch=args.arch) / 1e9,
                                                       " ".join("%.0f" % t for t in t_f), " ".join("%.0f" % t for t in t_a),
                                                       statistics.median(t_a) / statistics.median(t_f)), flush=True)
        del tf, ta, net_f, net_a
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
