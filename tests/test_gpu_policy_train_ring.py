"""The fused trainer on crowd rows (20..64 observed agents): FusedA3CTrainer(crowd=True), i.e. cavoid_policy_train /
cavoid_policy_train_regression on a crowd handle -- the ring forward kernels of cavoid_policy_train_ring.hpp, then the unchanged
policy_backward_kernel and the weight-gradient GEMMs.

The yardstick is float64 autograd of NetworkVP_rnn.loss (regression_loss for the supervised start's head); the criterion is
tests/policy_regimes.py's assert_gradients_match / assert_loss_matches, the project's one copy: as close to float64 as PyTorch's own
float32 autograd (x3), or 1e-4 of the gradient's largest entry.  Its relu-kink allowance needs B >= 8192 and no batch here is that large:
no row is excused.  beta = 3e-3, so that the entropy term is above the tolerances (policy_regimes' "beta" regime).

With R = 19 ring slots, M = 20 is the first refill, 38 a slot's second use, 39 the third lap, 63 and 64 the env's two widest rows."""
import copy
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

from tests import policy_regimes as R
from tests import regression_regimes as G

pytestmark = pytest.mark.gpu

RING = 19                                                   # kPolTrainRing = kPolMaxOthers
BETA = 3e-3


def _batch(net, B, seed, longest=None):
    """B rows clear of the relu kinks (policy_regimes.clear_of_relu_kinks, as build_case filters them) with num_other drawn per row from
    0 .. longest (default: M), one row of 0 and one of `longest` always among them (B = 1: the one row is full); y, a as build_case
    draws them"""
    M = net.max_others
    longest = M if longest is None else longest
    n = int(R.CANDIDATES * B) + 8
    x = R.inputs(net, n, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    x[:, 0] = torch.randint(0, longest + 1, (n,), generator=g).to(torch.float32).to(x.device)
    x[0, 0] = float(longest)
    if B > 1:
        x[1, 0] = 0.0
    clear = R.clear_of_relu_kinks(net, x)
    clear[:2] = True                                        # (the two pinned rows stay, whatever the band says: no row is excused anyway)
    x = x[clear][:B]
    assert x.shape[0] == B and float(x[:, 0].max()) == longest and (B == 1 or float(x[:, 0].min()) == 0.0)
    y = torch.randn(B, generator=g).to(x.device)
    a = torch.randint(0, net.num_actions, (B,), generator=g).to(x.device)
    return x, y, a


def _crowd_net(M, seed):
    net = R.build_net("rnn", M, seed=seed).cuda()
    net.beta = BETA
    return net


def _train_and_check(name, net, x, y, a, B):
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    total, _, _, want, torch32 = R.reference_gradients(net, x, y, a)
    tr = FusedA3CTrainer(net, learning_rate=0.0, crowd=True)
    assert tr.crowd and tr.policy.crowd
    loss = float(tr.train(x, y, a))
    report = []
    try:
        R.assert_loss_matches(loss, total)
        R.assert_gradients_match(net, want, torch32, B, report)
    finally:
        print("%s: loss %.6e (float64 %.6e)" % (name, loss, total))
        for k, err, err32, scale in report:
            print("    %-14s err %.2e  err32 %.2e  scale %.2e  err/scale %.1e" % (k, err, err32, scale, err / scale))
    return tr


@pytest.mark.parametrize("M", [20, 38, 39, 63, 64])
@pytest.mark.parametrize("B", [1, 63, 64, 130])
def test_ring_trainer_gradients_match_float64_autograd(M, B):
    net = _crowd_net(M, seed=20 + M)
    x, y, a = _batch(net, B, seed=1000 * M + B)
    _train_and_check("ring M=%d B=%d" % (M, B), net, x, y, a, B)


@pytest.mark.parametrize("M,longest", [(38, 11), (63, 30)])
def test_ring_trainer_when_no_row_is_full(M, longest):
    """the longest row is shorter than the ring / than M: the backward pass zero-fills gl and h_in for the steps no row took"""
    net = _crowd_net(M, seed=50 + M)
    x, y, a = _batch(net, 130, seed=7 * M, longest=longest)
    tr = _train_and_check("ring M=%d longest=%d" % (M, longest), net, x, y, a, 130)
    t, _ = tr._scratch(192)
    assert float(t["gl"][longest:].abs().max()) == 0.0 and float(t["h_in"][longest:].abs().max()) == 0.0


@pytest.mark.parametrize("M", [20, 63])
def test_ring_regression_head_matches_float64_autograd(M):
    """cavoid_policy_train_regression on a crowd handle, as tests/test_gpu_policy_regression.py holds the M <= 19 pair"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    B = 130
    net = _crowd_net(M, seed=G.NET_SEED + M)
    x, y, a = _batch(net, B, seed=300 + M)
    cost_p, cost_v, want, torch32 = G.reference_gradients(net, x, y, a)
    tr = FusedA3CTrainer(net, learning_rate=0.0, crowd=True)
    before = {k: t.detach().clone() for k, t in net.named_parameters()}
    got_p, got_v = tr.train_regression(x, y, a)
    got_p, got_v = float(got_p), float(got_v)
    report = []
    try:
        R.assert_loss_matches(got_p, cost_p)
        R.assert_loss_matches(got_v, cost_v)
        R.assert_gradients_match(net, want, torch32, B, report)
    finally:
        print("ring regression M=%d: cost_p %.6e (float64 %.6e)  cost_v %.6e (float64 %.6e)" % (M, got_p, cost_p, got_v, cost_v))
        for k, err, err32, scale in report:
            print("    %-14s err %.2e  err32 %.2e  scale %.2e  err/scale %.1e" % (k, err, err32, scale, err / scale))
    assert tr.training_step == 0 and all(torch.equal(t, before[k]) for k, t in net.named_parameters())


def test_ring_kernel_is_bitwise_the_narrow_kernel_on_narrow_rows():
    """One network's weights in an M = 19 network (policy_forward_kernel<4, true>) and an M = 24 one (the ring kernel); rows of <= 19
    observed agents, zero-padded.  Every row-local buffer of the pass is bit for bit the same, and the steps past 19 carry zero gradients.
    loss[2] is not row-local: twelve wavefronts add their sums to it with float atomics, in an order that changes from launch to launch
    (see tests/test_gpu_policy_regression.py on the bias gradients) -- it is held bitwise on the first 16 rows (one wavefront), and on the
    130 rows to what reordering twelve roundings of a float32 sum can move it: 12 x 2^-24 x sum |terms| <= 12 x 2^-24 x the two sums'
    own magnitude (every term of cost_v is >= 0; cost_p's terms are of one sign up to the 3e-3 entropy share)."""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    B = 130
    narrow, wide = _crowd_net(19, seed=5), _crowd_net(24, seed=5)
    with torch.no_grad():
        for name, prm in narrow.named_parameters():
            getattr(wide, name).copy_(prm)
        wide.avg[:narrow.input_size].copy_(narrow.avg)
        wide.std[:narrow.input_size].copy_(narrow.std)
    x19, y, a = _batch(narrow, B, seed=3)
    x24 = torch.zeros((B, wide.input_size), device="cuda")
    x24[:, :narrow.input_size] = x19
    tn, tw = FusedA3CTrainer(narrow, learning_rate=0.0), FusedA3CTrainer(wide, learning_rate=0.0, crowd=True)
    assert not tn.crowd and tw.crowd
    a32 = a.to(torch.int32)
    for n in (B, 16):
        bn = {k: v.clone() for k, v in tn._pass(x19[:n].contiguous(), y[:n].contiguous(), a32[:n].contiguous(), n).items()}
        bw = {k: v.clone() for k, v in tw._pass(x24[:n].contiguous(), y[:n].contiguous(), a32[:n].contiguous(), n).items()}
        for k in ("gh", "z1", "z2", "z3", "g1", "g2", "g3", "l1_in"):
            assert torch.equal(bn[k], bw[k]), (n, k)
        assert torch.equal(bn["gl"], bw["gl"][:19]) and torch.equal(bn["h_in"], bw["h_in"][:19]), n
        assert float(bw["gl"][19:].abs().max()) == 0.0, n
        if n == 16:
            assert torch.equal(bn["loss"], bw["loss"])
        else:
            bound = 12.0 * 2.0 ** -24 * bn["loss"].abs()
            assert ((bn["loss"] - bw["loss"]).abs() <= bound).all(), (bn["loss"], bw["loss"])


def test_ring_trainer_batch_rounding():
    """2048 + 100 rows: the buffers round up to 4096 rows (tiles past the batch carry zero gradients), the weight-gradient GEMMs are
    split-K, the LSTM's over 31 x 4096 rows"""
    M, B = 31, 2048 + 100
    net = _crowd_net(M, seed=77)
    x, y, a = _batch(net, B, seed=4242)
    tr = _train_and_check("ring M=31 B=2148", net, x, y, a, B)
    assert list(tr._buffers) == [4096]
    assert float(tr._scratch(4096)[0]["gh"][B:].abs().max()) == 0.0


def test_ring_trainer_learns_like_the_autograd_trainer():
    """five Adam steps from equal weights, under the bounds of tests/test_gpu_policy_ws.py's test of the same comparison; the trainer's
    FusedPolicy then acts on the updated weights (tests/test_gpu_policy_crowd.py's forward bounds)"""
    from rl_collision_avoidance_amd.ga3c.network import A3CTrainer
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    from tests.policy_support import P_TOL, V_TOL
    M, B = 31, 256
    net_a = _crowd_net(M, seed=31)
    net_b = copy.deepcopy(net_a)
    start = {k: t.detach().clone() for k, t in net_a.named_parameters()}
    ta, tb = A3CTrainer(net_a, learning_rate=1e-4), FusedA3CTrainer(net_b, learning_rate=1e-4, crowd=True)
    for step in range(5):
        x, y, a = _batch(net_a, B, seed=100 + step)
        la = ta.train(x, y, torch.nn.functional.one_hot(a, 11).float())
        lb = float(tb.train(x, y, a))
        assert abs(la - lb) <= 1e-3 * max(1.0, abs(la))
    assert tb.training_step == 5
    for (k, pa), (_, pb) in zip(net_a.named_parameters(), net_b.named_parameters()):
        d = (pa - pb).abs()
        assert (d > 2e-5).float().mean().item() <= 1e-3 and d.max().item() <= 1e-4, (k, d.max().item(), int((d > 2e-5).sum()))
        assert not torch.equal(pb, start[k]), k
    x, _, _ = _batch(net_b, 130, seed=9)
    p, v = tb.policy(x)
    with torch.no_grad():
        _, p_ref, v_ref = net_b.forward(x)
    assert (p - p_ref).abs().max().item() <= P_TOL
    assert ((v - v_ref).abs() <= V_TOL + V_TOL * v_ref.abs()).all()


def test_crowd_training_stays_opt_in():
    """the default keeps refusing rows above 19 observed agents, word for word (tests/test_gpu_policy_crowd.py pins the same); weight-sharing
    networks above 19 are refused with or without crowd=True; the C ABI's argument checks hold on a crowd handle"""
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    net = _crowd_net(20, seed=1)
    with pytest.raises(ValueError, match="19"):
        FusedA3CTrainer(net)
    with pytest.raises(ValueError, match="the fused trainer carries up to 19 observed neighbours"):
        FusedA3CTrainer(net, crowd=False)
    ws = R.build_net("weight_sharing", 20, seed=1).cuda()
    for crowd in (False, True):
        with pytest.raises(ValueError):
            FusedA3CTrainer(ws, crowd=crowd)
    tr = FusedA3CTrainer(net, crowd=True)
    _, good = tr._scratch(64)
    p = lambda t: C.c_void_p(t.data_ptr())
    x = torch.zeros((65, net.input_size), device="cuda")
    y, a = torch.zeros(65, device="cuda"), torch.zeros(65, dtype=torch.int32, device="cuda")
    lib, h = tr.policy._lib, tr.policy._h
    bad = _lib.CavoidPolicyTrainBuffers.from_buffer_copy(good)
    bad.struct_size = C.sizeof(_lib.CavoidPolicyTrainBuffers) - 8
    assert lib.cavoid_policy_train(h, p(x), 64, net.input_size, p(y), p(a), 1e-4, 1e-6, C.byref(bad), None) == -1
    assert lib.cavoid_policy_train(h, p(x), 65, net.input_size, p(y), p(a), 1e-4, 1e-6, C.byref(good), None) == -1     # capacity_rows < rows
    assert lib.cavoid_policy_train(h, p(x), 64, net.input_size - 1, p(y), p(a), 1e-4, 1e-6, C.byref(good), None) == -1  # stride < row
    assert lib.cavoid_policy_train(h, p(x), 64, net.input_size, p(y), p(a), 1e-4, 1e-6, C.byref(good), None) == 0
    assert lib.cavoid_policy_train_regression(h, p(x), 64, net.input_size, p(y), p(a), C.byref(good), None) == 0
    torch.cuda.synchronize()
