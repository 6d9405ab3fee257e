"""Shared helpers of the tests of the supervised start's loss head (cost_regression, NetworkVPCore.py:90-100,123): a plain module,
as tests/policy_regimes.py is for the A3C head.  tests/test_gpu_policy_regression.py (GPU) and tests/test_policy_regression_host.py
(CPU) build the SAME cases from it, so that what the host test shows about a case -- the row filter excludes few rows, a wrong head
would move the gradients far beyond the criterion's bound -- holds for the batch the kernels are run on.

The yardstick is ``ga3c.regression.regression_loss`` under float64 autograd; the criterion is policy_regimes.assert_gradients_match
(as close to float64 as PyTorch's own float32 autograd on the same loss, x3, or 1e-4 of the gradient's largest entry) and
policy_regimes.assert_loss_matches for each of the two loss sums.  Nothing here adds a tolerance.

The regimes, each on the four networks of policy_regimes.ARCH_M at B = 1000 (not a multiple of 64) and B = 8192:
  fresh       freshly initialised weights;
  min_policy  MIN_POLICY = 0.02: cost_regression takes the logits, so the floor must play no part;
  gain40      the p head x 40 (policy_regimes.GAIN_TRAINER): selected probabilities far below LOG_EPSILON, which must play no part;
  gain150     the p head x 150 (GAIN_DRAW): the selected float32 softmax entry is exactly 0 in a good share of the rows.
"""
import collections
import copy

import torch

from tests import policy_regimes as R

NET_SEED, INPUT_SEED = 7, 3
REGIMES = {"fresh": (0.0, 0.0), "min_policy": (0.02, 0.0), "gain40": (0.0, R.GAIN_TRAINER), "gain150": (0.0, R.GAIN_DRAW)}
Case = collections.namedtuple("Case", "regime arch M B min_policy gain A")
CASES = [Case(regime, arch, M, B, mp, gain, 11) for regime, (mp, gain) in REGIMES.items() for arch, M in R.ARCH_M for B in (1000, 8192)]
MIN_ZERO_SELECTED = 0.10   # condition of gain150: at least this share of the rows select a float32 softmax entry that is exactly 0


def case_id(c):
    return "%s-%s%d-B%d%s" % (c.regime, "ws" if c.arch == "weight_sharing" else "rnn", c.M, c.B, "-A%d" % c.A if c.A != 11 else "")


def build_case(case, device="cpu"):
    """(net, x [B], y [B], a [B], info): the network in its regime, the first B of 1.25 B candidate rows that are clear of the relu
    kinks, random teacher actions and randn value targets.  Everything is drawn on the CPU, so every device sees the same batch."""
    net = R.build_net(case.arch, case.M, seed=NET_SEED, min_policy=case.min_policy, A=case.A)
    if case.gain:
        R.confident(net, case.gain)
    n = int(R.CANDIDATES * case.B)
    x = R.inputs(net, n, seed=INPUT_SEED)
    g = torch.Generator().manual_seed(case.B)
    y = torch.randn(n, generator=g)
    a = torch.randint(0, case.A, (n,), generator=g)
    clear = R.clear_of_relu_kinks(net, x)
    keep = torch.nonzero(clear).flatten()[:case.B]
    x, y, a = x[keep], y[keep], a[keep]
    with torch.no_grad():
        _, p32, _ = net.forward(x)
    info = {"rows": int(keep.numel()), "excluded": 1.0 - clear.float().mean().item(),
            "zero_selected": (p32.gather(1, a.unsqueeze(1)) == 0.0).float().mean().item()}
    return net.to(device), x.to(device), y.to(device), a.to(device), info


def assert_conditions(case, info):
    """Conditions on a case's batch, fixed before any kernel ran.  If a seed misses one, another seed is picked; the condition stays."""
    assert info["rows"] == case.B, (case, info)
    assert info["excluded"] <= R.MAX_EXCLUDED, (case, info)
    if case.regime == "gain150":
        assert info["zero_selected"] >= MIN_ZERO_SELECTED, (case, info)


def reference_gradients(net, x, y, a):
    """float64 autograd of regression_loss (the yardstick) and PyTorch's float32 autograd of it on the same rows:
    (cost_p64, cost_v64, {name: grad64}, {name: grad32})"""
    from rl_collision_avoidance_amd.ga3c.regression import regression_loss
    ref_net = copy.deepcopy(net).double()
    ref_net.zero_grad()
    total, cost_p, cost_v = regression_loss(ref_net, x.double(), y.double(), a)
    total.backward()
    want = {k: t.grad.clone() for k, t in ref_net.named_parameters()}
    net.zero_grad()
    regression_loss(net, x, y, a)[0].backward()
    torch32 = {k: t.grad.clone() for k, t in net.named_parameters()}
    net.zero_grad()
    return float(cost_p.detach()), float(cost_v.detach()), want, torch32


# ---- the head written out (float64, CPU), and what a wrong one would do ------------------------------------------------------
MUTATIONS = ("min_policy_softmax", "a3c_log_clamp", "no_value_term")


def head_gradients(net, x, y, a, mutation=None):
    """{name: float64 gradient} of the loss whose gradient at the head columns is the regression head's own formula,
        g_k = softmax(z)_k - [k == a]  (k < A),    g_A = v - y,
    or, with one of MUTATIONS, of the wrong head it names: cross-entropy on p' = (softmax + MIN_POLICY) / (1 + A MIN_POLICY) instead
    of on the logits; the A3C head's log(max(p_a, LOG_EPSILON)); no value term."""
    assert mutation is None or mutation in MUTATIONS
    net64 = copy.deepcopy(net).double()
    net64.zero_grad()
    onehot = torch.nn.functional.one_hot(a.long(), net64.num_actions).double()
    logits, p, v = net64.forward(x.double())                   # p = (softmax + MIN_POLICY) * scale
    value = torch.zeros((), dtype=torch.float64) if mutation == "no_value_term" else ((v - y.double()).detach() * v).sum()
    if mutation == "min_policy_softmax":
        policy = -torch.log((p * onehot).sum(dim=1)).sum()
    elif mutation == "a3c_log_clamp":
        sel = (torch.softmax(logits, dim=1) * onehot).sum(dim=1)
        policy = -torch.log(torch.clamp_min(sel, net64.log_epsilon)).sum()
    else:
        policy = (logits * (torch.softmax(logits, dim=1) - onehot).detach()).sum()
    (policy + value).backward()
    return {k: (t.grad.clone() if t.grad is not None else torch.zeros_like(t)) for k, t in net64.named_parameters()}


def worst_ratio(got, want, torch32):
    """max over the parameters of |got - want| / (the bound assert_gradients_match allows that parameter)"""
    worst = 0.0
    for k, ref in want.items():
        scale = ref.abs().max().item() + 1e-6
        err32 = (torch32[k].double() - ref).abs().max().item()
        worst = max(worst, (got[k] - ref).abs().max().item() / max(3.0 * err32, 1e-4 * scale))
    return worst
