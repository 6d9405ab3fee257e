"""What the GPU tests of the fused policy kernels share: the tolerances against the PyTorch float32 graph, a network with every bias path
live, inputs around the network's normalisation, and the bit-identity check of the tile-to-wavefront forms.  A plain module: pytest
does not rewrite its asserts, so each carries its own message."""
import torch

P_TOL = 2e-5       # softmax probabilities (absolute; p <= 1): f32 MFMA vs rocBLAS f32, different summation order
V_TOL = 2e-4       # value head (|v| = O(1)); absolute + relative


def _net(M, seed=0, min_policy=0.0, normalize=True, A=11):
    from rl_collision_avoidance_amd.config import EnvConfig
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = M + 1
            EnvConfig.__init__(self)
    cfg = Cfg()
    cfg.MIN_POLICY = min_policy
    cfg.NORMALIZE_INPUT = normalize
    net = NetworkVP_rnn(cfg, num_actions=A, seed=seed).cuda()
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():                      # non-zero biases so that every bias path is exercised
        for name, prm in net.named_parameters():
            if name.endswith("_bias"):
                prm.copy_((torch.rand(prm.shape, generator=g) - 0.5).to(prm.device))
    return net


def _inputs(net, B, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    M = net.max_others
    x = torch.randn((B, net.input_size), generator=g) * scale * net.std.cpu() + net.avg.cpu()
    x[:, 0] = torch.randint(0, M + 1, (B,), generator=g).to(torch.float32)
    return x.cuda()


def _check_forms_bit_identical(net, x, M, B, form, monkeypatch):
    """the body of test_gpu_policy.py::test_other_tile_to_wavefront_forms_are_bit_identical (tests/test_gpu_policy_loss_heads.py runs it
    on a confident network too); returns the default form's probabilities"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    tag = (form, M, B)
    g = torch.Generator().manual_seed(3)
    x[:, 0] = torch.randint(0, M + 1, (B,), generator=g).float().cuda()
    x[: B // 3, 0] = float(M)                               # tiles in which every row is live at every LSTM step
    x[B // 3: B // 3 + 70, 0] = 1.0                         # ... and a tile with fewer steps than its neighbour (duo: the idle barrier pairs)
    monkeypatch.setenv("CAVOID_POLICY_FORM", "quad")
    pol4 = FusedPolicy(net, seed=77)
    monkeypatch.setenv("CAVOID_POLICY_FORM", form)
    pol8 = FusedPolicy(net, seed=77)
    a4, p4, v4 = pol4.act(x)
    a8, p8, v8 = pol8.act(x)
    for name, u, v in (("p", p4, p8), ("v", v4, v8), ("actions", a4, a8)):
        assert torch.equal(u, v), (tag, "full pass", name)
    assert float((p4.sum(dim=1) - 1.0).abs().max()) < 1e-5, (tag, "probabilities sum to", float((p4.sum(dim=1) - 1.0).abs().max()))
    assert B < 100 or a4.float().std().item() > 0, (tag, "every row drew the same action")
    idx = torch.zeros(B, dtype=torch.int32, device="cuda")
    listed = torch.randperm(B, generator=torch.Generator().manual_seed(1))[: B // 2 + 3].to(torch.int32).cuda()
    idx[: listed.numel()] = listed
    count = torch.tensor([listed.numel()], dtype=torch.int32, device="cuda")
    a4r, p4r, v4r = pol4.act(x, rows=(idx, count))
    a8r, p8r, v8r = pol8.act(x, rows=(idx, count))
    for name, u, v in (("p", p4r, p8r), ("v", v4r, v8r), ("actions", a4r, a8r)):
        assert torch.equal(u, v), (tag, "row-list pass", name)
    count.zero_()                                            # an empty list: every workgroup leaves at once
    a0, p0, v0 = pol8.act(x, rows=(idx, count))
    assert float(p0.abs().sum()) == 0.0, (tag, "empty row list wrote probabilities", float(p0.abs().sum()))
    return p4
