"""Time the fused policy kernel against the PyTorch-ROCm graph of the same network (development aid).
usage: python tools/polbench.py [rows] [max_other] [--arch rnn|weight_sharing]
  (max_other 1..64: above 19 the rnn handle runs the crowd kernel, cavoid_policy_crowd.hpp; weight_sharing: 1..19 on cavoid_policy_ws.hpp,
   20..64 on the ring kernel of cavoid_policy_wsring.hpp, FusedPolicy(ws_crowd=True))
Every row observes max_other agents.  fused_us: predict + sampled select_action (act); forward_us: predict only; torch_us: predict_p_and_v."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from rl_collision_avoidance_amd.config import EnvConfig
from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
from rl_collision_avoidance_amd.ga3c.policy_kernel import MAX_OTHERS_WS, FusedPolicy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rows", type=int, nargs="?", default=32768)
    ap.add_argument("max_other", type=int, nargs="?", default=3)
    ap.add_argument("--arch", default="rnn", choices=["rnn", "weight_sharing"])
    args = ap.parse_args()
    B, M = args.rows, args.max_other

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = M + 1
            EnvConfig.__init__(self)
    net = NetworkVP_rnn(Cfg(), arch=args.arch).cuda()
    pol = FusedPolicy(net, ws_crowd=M > MAX_OTHERS_WS)
    g = torch.Generator().manual_seed(0)
    x = (torch.randn((B, net.input_size), generator=g) * net.std.cpu() + net.avg.cpu())
    x[:, 0] = float(M)
    x = x.cuda()

    def timeit(fn, n=50):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n
    t_fused = timeit(lambda: pol.act(x))
    t_forward = timeit(lambda: pol(x))
    t_torch = timeit(lambda: net.predict_p_and_v(x))
    t_load = timeit(pol.refresh)
    chunks = (1 + 5 * (M - 1)) + 5 + 16 + 16 if args.arch == "rnn" else 4.25 * M + 1 + 16 + 16   # (ws: the filter is a quarter chunk per slot)
    flop = B * (chunks * 16 * 256 * 2 + 256 * 16 * 2)
    if args.arch == "rnn":
        useful = B * 2 * ((7 + 64 * (M - 1) + 7 * (M - 1)) * 256 + 68 * 256 + 2 * 256 * 256 + 256 * 12)
    else:
        useful = B * 2 * (M * 8 * 64 + (4 + 64 * M) * 256 + 2 * 256 * 256 + 256 * 12)
    form = ("wsring" if pol.crowd else "ws") if pol.ws else ("crowd" if pol.crowd else os.environ.get("CAVOID_POLICY_FORM", "quad"))
    print({"form": form, "products": pol.inference_form[1], "rows": B, "max_other": M, "fused_us": round(t_fused, 1), "forward_us": round(t_forward, 1),
           "torch_us": round(t_torch, 1), "speedup_act": round(t_torch / t_fused, 2), "pack_us": round(t_load, 1),
           "issued_TFLOPs": round(flop / t_fused * 1e-6, 1), "useful_TFLOPs": round(useful / t_fused * 1e-6, 1),
           "frac_of_157TF_issued": round(flop / t_fused * 1e-6 / 157.3, 3)})


if __name__ == "__main__":
    main()
