"""The weight-sharing network on rows of 20..64 observed neighbours: FusedPolicy(ws_crowd=True) / FusedA3CTrainer(ws_crowd=True), i.e. the
ring kernels of cavoid_policy_wsring.hpp on a cavoid_policy_create_ws_crowd handle -- inference, the launch contract (row list, strided
rows, the action draw, hipGraph), the trainer pass with either loss head in front of the unchanged policy_ws_backward_kernel, and the
refusals that stay.

Yardsticks: PyTorch's float32 graph under tests/test_gpu_policy.py's P_TOL / V_TOL and the float64 network for inference; float64
autograd of NetworkVP_rnn.loss (regression_loss for the supervised start's head) under tests/policy_regimes.py's assert_gradients_match /
assert_loss_matches for the trainer -- its relu-kink allowance needs B >= 8192 and no batch here is that large: no row is excused.
beta = 3e-3, so that the entropy term is above the tolerances.

With R = 19 ring slots, M = 20 is the first refill, 38 fills every slot a second time, 39 starts a third lap, 63 and 64 are the env's two
widest rows; B = 1, 63, 64, 130: a partial tile, a full one, a third tile with two rows.

The batches: int(1.25 B) + 8 candidate rows, counts drawn over 0..longest, row 0 pinned full and row 1 at 0, filtered by
clear_of_relu_kinks.  Two conditions, neither a measurement: the candidates yield B clear rows, and the two pinned rows are themselves
clear (asserted, not forced).  Every seed below was checked against both on the CPU; if one is changed, the conditions stay."""
import copy
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

from tests import policy_regimes as R
from tests import regression_regimes as G

pytestmark = pytest.mark.gpu

BETA = 3e-3
MS, BS = (20, 38, 39, 63, 64), (1, 63, 64, 130)


def _batch(net, B, seed, longest=None):
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
    assert bool(clear[:2].all()), "a pinned row lies in the relu band: pick another seed"
    x = x[clear][:B]
    assert x.shape[0] == B and float(x[:, 0].max()) == longest and (B == 1 or float(x[:, 0].min()) == 0.0)
    y = torch.randn(B, generator=g).to(x.device)
    a = torch.randint(0, net.num_actions, (B,), generator=g).to(x.device)
    return x, y, a


def _ws_net(M, seed):
    net = R.build_net("weight_sharing", M, seed=seed).cuda()
    net.beta = BETA
    return net


_cases = {}


def _case(M, B):
    """the (M, B) network and batch, shared by the inference and the trainer test (never modified: learning_rate = 0)"""
    if (M, B) not in _cases:
        net = _ws_net(M, seed=20 + M)
        _cases[(M, B)] = (net,) + _batch(net, B, seed=1000 * M + B + 28)
    return _cases[(M, B)]


def _check32(p, v, p_ref, v_ref):
    from tests.policy_support import P_TOL, V_TOL
    assert torch.isfinite(p).all() and torch.isfinite(v).all()
    assert (p - p_ref).abs().max().item() <= P_TOL
    assert ((v - v_ref).abs() <= V_TOL + V_TOL * v_ref.abs()).all()


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("B", BS)
def test_wsring_forward_matches_torch_fp32_and_float64(M, B):
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    net, x, _, _ = _case(M, B)
    pol = FusedPolicy(net, ws_crowd=True)
    assert pol.crowd and pol.ws and pol.inference_form == ("f32", 0)
    p, v = pol(x)
    with torch.no_grad():
        _, p32, v32 = net.forward(x)
    p64, v64 = R.forward64(net, x)
    assert p.shape == (B, 11) and v.shape == (B,)
    _check32(p, v, p32, v32)
    assert (p.sum(dim=1) - 1.0).abs().max().item() <= 1e-5
    e_p, e_torch_p = (p.double() - p64).abs().max().item(), (p32.double() - p64).abs().max().item()
    e_v, e_torch_v = (v.double() - v64).abs().max().item(), (v32.double() - v64).abs().max().item()
    print("wsring M=%d B=%d: |dp| %.2e (torch f32 %.2e)  |dv| %.2e (torch f32 %.2e)" % (M, B, e_p, e_torch_p, e_v, e_torch_v))
    # the weight-sharing kernel's bar (tests/test_gpu_policy_ws.py), or assert_gradients_match's rule: a layer1 dot product of 4 100
    # terms has not been measured against that bar
    assert e_p <= max(1e-6, 3.0 * e_torch_p) and e_v <= max(5e-6, 3.0 * e_torch_v)
    pol.close()


def _launch_case():
    net = _ws_net(38, seed=51)
    return net, R.inputs(net, 2000, seed=6)


def test_wsring_row_list_pass_equals_the_full_pass_on_the_listed_rows():
    """... and is zero elsewhere: the ring's refill goes through the tile's row list"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    net, x = _launch_case()
    B = x.shape[0]
    listed = torch.randperm(B, generator=torch.Generator().manual_seed(1))[:1234].to(torch.int32).cuda()
    index = torch.zeros(B, dtype=torch.int32, device="cuda")
    index[:listed.numel()] = listed
    count = torch.tensor([listed.numel()], dtype=torch.int32, device="cuda")
    pol = FusedPolicy(net, seed=77, ws_crowd=True)
    a_full, p_full, v_full = pol.act(x)
    with torch.no_grad():
        _, p_ref, v_ref = net.forward(x)
    _check32(p_full, v_full, p_ref, v_ref)
    pol.seed(77)
    a_rows, p_rows, v_rows = pol.act(x, rows=(index, count))
    sel = listed.long()
    assert torch.equal(p_rows[sel], p_full[sel]) and torch.equal(v_rows[sel], v_full[sel]) and torch.equal(a_rows[sel], a_full[sel])
    rest = torch.ones(B, dtype=torch.bool, device="cuda")
    rest[sel] = False
    assert float(p_rows[rest].abs().sum()) == 0.0 and float(v_rows[rest].abs().sum()) == 0.0
    count.zero_()
    _, p0, _ = pol.act(x, rows=(index, count))
    assert float(p0.abs().sum()) == 0.0


def test_wsring_strided_rows_draw_and_hip_graph():
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    net, x = _launch_case()
    B = x.shape[0]
    pol = FusedPolicy(net, seed=21, ws_crowd=True)
    p, v = pol(x)
    # a strided view of wider rows (as the env's observation tensor is read in place)
    wide = torch.full((B, net.input_size + 3), 7.0, device="cuda")
    wide[:, 1:1 + net.input_size] = x
    view = wide[:, 1:1 + net.input_size]
    assert not view.is_contiguous()
    p_s, v_s = pol(view)
    assert torch.equal(p_s, p) and torch.equal(v_s, v)
    # greedy is argmax; a reseeded draw repeats
    a_g, p_g, _ = pol.act(x, greedy=True)
    assert torch.equal(a_g.long(), p_g.argmax(dim=1))
    pol.seed(21)
    want = [pol.act(x)[0].clone() for _ in range(3)]
    assert not torch.equal(want[0], want[1])
    assert int(want[0].min()) >= 0 and int(want[0].max()) < net.num_actions
    pol.seed(21)
    assert torch.equal(pol.act(x)[0], want[0])
    # a captured act replayed 3 times = 3 eager calls
    cap = FusedPolicy(net, seed=21, ws_crowd=True)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            a, _, _ = cap.act(x)
    torch.cuda.synchronize()
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, want[k]), k


def _train_and_check(name, net, x, y, a, B):
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    total, _, _, want, torch32 = R.reference_gradients(net, x, y, a)
    tr = FusedA3CTrainer(net, learning_rate=0.0, ws_crowd=True)
    assert tr.ws and tr.ws_crowd and tr.policy.crowd and not tr.crowd
    loss = float(tr.train(x, y, a))
    report = []
    try:
        assert "other_kernel" in want and set(want) == {k for k, _ in net.named_parameters()}
        R.assert_loss_matches(loss, total)
        R.assert_gradients_match(net, want, torch32, B, report)
    finally:
        print("%s: loss %.6e (float64 %.6e)" % (name, loss, total))
        for k, err, err32, scale in report:
            print("    %-14s err %.2e  err32 %.2e  scale %.2e  err/scale %.1e" % (k, err, err32, scale, err / scale))
    return tr


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("B", BS)
def test_wsring_trainer_gradients_match_float64_autograd(M, B):
    net, x, y, a = _case(M, B)
    _train_and_check("wsring M=%d B=%d" % (M, B), net, x, y, a, B)


@pytest.mark.parametrize("M,longest", [(38, 11), (63, 30)])
def test_wsring_trainer_on_short_rows(M, longest):
    """weight-sharing runs every slot whatever the count: is_on of the refilled slots is 0 in every row"""
    net = _ws_net(M, seed=50 + M)
    x, y, a = _batch(net, 130, seed=7 * M, longest=longest)
    tr = _train_and_check("wsring M=%d longest=%d" % (M, longest), net, x, y, a, 130)
    t, _ = tr._scratch(192)
    assert float(t["f_in"][longest:, :, 7].abs().max()) == 0.0
    assert float(t["f_in"][:longest, :130, 7].max()) == 1.0


@pytest.mark.parametrize("M", [20, 63])
def test_wsring_regression_head_matches_float64_autograd(M):
    """cavoid_policy_train_regression_ws on a ws-crowd handle, as tests/test_gpu_policy_regression.py holds the M <= 19 pair"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    B = 130
    net = _ws_net(M, seed=G.NET_SEED + M)
    x, y, a = _batch(net, B, seed=300 + M)
    cost_p, cost_v, want, torch32 = G.reference_gradients(net, x, y, a)
    tr = FusedA3CTrainer(net, learning_rate=0.0, ws_crowd=True)
    before = {k: t.detach().clone() for k, t in net.named_parameters()}
    got_p, got_v = tr.train_regression(x, y, a)
    got_p, got_v = float(got_p), float(got_v)
    report = []
    try:
        R.assert_loss_matches(got_p, cost_p)
        R.assert_loss_matches(got_v, cost_v)
        R.assert_gradients_match(net, want, torch32, B, report)
    finally:
        print("wsring regression M=%d: cost_p %.6e (float64 %.6e)  cost_v %.6e (float64 %.6e)" % (M, got_p, cost_p, got_v, cost_v))
        for k, err, err32, scale in report:
            print("    %-14s err %.2e  err32 %.2e  scale %.2e  err/scale %.1e" % (k, err, err32, scale, err / scale))
    assert tr.training_step == 0 and all(torch.equal(t, before[k]) for k, t in net.named_parameters())


def test_wsring_kernels_are_bitwise_the_narrow_kernels_on_narrow_rows():
    """One network's weights in an M = 19 network (policy_ws_forward_kernel) and an M = 24 one (the ring kernels) whose layer1 rows for
    slots 19..23 are zero; the input rows padded with arbitrary finite values in those slots.  A premature or misplaced refill would put
    another slot's values in front of slots 0..4's filter.  Inference: p, v and the drawn actions bit for bit, full pass and row-list pass.
    Trainer: every row-local buffer bit for bit, gf of the slots past 19 exactly 0.  loss[2] is not row-local (float atomics of twelve
    wavefronts, in a launch-dependent order): bitwise on 16 rows (one tile, one wavefront's rows), on the 130 rows within
    12 x 2^-24 x |loss| -- the bound tests/test_gpu_policy_train_ring.py derives."""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer, FusedPolicy
    B = 130
    narrow, wide = _ws_net(19, seed=5), _ws_net(24, seed=5)
    w19 = narrow.layer1_kernel.shape[0]
    with torch.no_grad():
        for name, prm in narrow.named_parameters():
            if name == "layer1_kernel":
                wide.layer1_kernel.zero_()
                wide.layer1_kernel[:w19].copy_(prm)
            else:
                getattr(wide, name).copy_(prm)
        wide.avg.zero_()
        wide.std.fill_(1.0)
        wide.avg[:narrow.input_size].copy_(narrow.avg)
        wide.std[:narrow.input_size].copy_(narrow.std)
    x19, y, a = _batch(narrow, B, seed=3)
    x24 = 3.0 * torch.randn((B, wide.input_size), generator=torch.Generator().manual_seed(11)).cuda() - 1.0
    x24[:, :narrow.input_size] = x19
    # inference
    pn, pw = FusedPolicy(narrow, seed=9), FusedPolicy(wide, seed=9, ws_crowd=True)
    assert not pn.crowd and pw.crowd
    a_n, p_n, v_n = pn.act(x19)
    a_w, p_w, v_w = pw.act(x24)
    assert torch.equal(p_n, p_w) and torch.equal(v_n, v_w) and torch.equal(a_n, a_w)
    listed = torch.randperm(B, generator=torch.Generator().manual_seed(2))[:71].to(torch.int32).cuda()
    index = torch.zeros(B, dtype=torch.int32, device="cuda")
    index[:71] = listed
    count = torch.tensor([71], dtype=torch.int32, device="cuda")
    r_n, r_w = pn.act(x19, rows=(index, count)), pw.act(x24, rows=(index, count))
    assert all(torch.equal(u, w) for u, w in zip(r_n, r_w))
    assert torch.equal(r_w[1][listed.long()], p_w[listed.long()])
    # trainer pass
    tn, tw = FusedA3CTrainer(narrow, pn, learning_rate=0.0), FusedA3CTrainer(wide, pw, learning_rate=0.0)   # (a ws-crowd policy is enough)
    assert not tn.ws_crowd and tw.ws_crowd
    a32 = a.to(torch.int32)
    for n in (B, 16):
        bn = {k: t.clone() for k, t in tn._pass(x19[:n].contiguous(), y[:n].contiguous(), a32[:n].contiguous(), n).items()}
        bw = {k: t.clone() for k, t in tw._pass(x24[:n].contiguous(), y[:n].contiguous(), a32[:n].contiguous(), n).items()}
        for k in ("gh", "z1", "z2", "z3", "g1", "g2", "g3"):
            assert torch.equal(bn[k], bw[k]), (n, k)
        assert torch.equal(bn["l1_in"], bw["l1_in"][:, :w19]), n
        assert torch.equal(bn["f_in"], bw["f_in"][:19]) and torch.equal(bn["gf"], bw["gf"][:19]), n
        assert float(bw["gf"][19:].abs().max()) == 0.0, n
        assert float(bw["f_in"][19:, :n, :7].abs().max()) > 0.0      # (the padded slots did go through the ring)
        if n == 16:
            assert torch.equal(bn["loss"], bw["loss"])
        else:
            bound = 12.0 * 2.0 ** -24 * bn["loss"].abs()
            assert ((bn["loss"] - bw["loss"]).abs() <= bound).all(), (bn["loss"], bw["loss"])


def test_wsring_trainer_batch_rounding():
    """2048 + 100 rows: the buffers round up to 4096 rows (tiles past the batch carry zero gradients), the weight-gradient GEMMs are
    split-K, the filter's over 31 x 4096 rows"""
    M, B = 31, 2048 + 100
    net = _ws_net(M, seed=77)
    x, y, a = _batch(net, B, seed=4242)
    tr = _train_and_check("wsring M=31 B=2148", net, x, y, a, B)
    assert list(tr._buffers) == [4096]
    assert float(tr._scratch(4096)[0]["gh"][B:].abs().max()) == 0.0


def test_wsring_trainer_learns_like_the_autograd_trainer():
    """five Adam steps from equal weights, under the bounds of tests/test_gpu_policy_ws.py's test of the same comparison; the trainer's
    FusedPolicy then acts on the updated weights"""
    from rl_collision_avoidance_amd.ga3c.network import A3CTrainer
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    M, B = 31, 256
    net_a = _ws_net(M, seed=31)
    net_b = copy.deepcopy(net_a)
    start = {k: t.detach().clone() for k, t in net_a.named_parameters()}
    batches = [_batch(net_a, B, seed=100 + step) for step in range(5)]      # (filtered on the starting weights, the ones the seeds were checked on)
    ta, tb = A3CTrainer(net_a, learning_rate=1e-4), FusedA3CTrainer(net_b, learning_rate=1e-4, ws_crowd=True)
    for x, y, a in batches:
        la = ta.train(x, y, torch.nn.functional.one_hot(a, 11).float())
        lb = float(tb.train(x, y, a))
        assert abs(la - lb) <= 1e-3 * max(1.0, abs(la))
    assert tb.training_step == 5
    for (k, pa), (_, pb) in zip(net_a.named_parameters(), net_b.named_parameters()):
        d = (pa - pb).abs()
        assert (d > 2e-5).float().mean().item() <= 1e-3 and d.max().item() <= 1e-4, (k, d.max().item(), int((d > 2e-5).sum()))
        assert not torch.equal(pb, start[k]), k
    x = R.inputs(net_b, 130, seed=9)
    p, v = tb.policy(x)
    with torch.no_grad():
        _, p_ref, v_ref = net_b.forward(x)
    _check32(p, v, p_ref, v_ref)


def test_wsring_stays_opt_in_and_refuses_what_it_should():
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer, FusedPolicy
    ws20 = _ws_net(20, seed=1)
    with pytest.raises(ValueError, match="19"):
        FusedPolicy(ws20)
    for crowd in (False, True):
        with pytest.raises(ValueError):
            FusedA3CTrainer(ws20, crowd=crowd)
    small = FusedPolicy(_ws_net(7, seed=1), ws_crowd=True)
    assert small.ws and not small.crowd                      # an ordinary cavoid_policy_create_ws handle
    h = C.c_void_p()
    assert small._lib.cavoid_policy_create_ws_crowd(19, 11, 0, C.byref(h)) == -4 and not h.value
    assert small._lib.cavoid_policy_create_ws_crowd(65, 11, 0, C.byref(h)) == -1 and not h.value
    tr = FusedA3CTrainer(ws20, ws_crowd=True)
    lib, hd = tr.policy._lib, tr.policy._h
    p = lambda t: C.c_void_p(t.data_ptr())
    w = _lib.CavoidPolicyWeights()
    w.struct_size = C.sizeof(_lib.CavoidPolicyWeights)
    assert lib.cavoid_policy_load(hd, C.byref(w), None) == -1                      # an LSTM load on a weight-sharing handle
    lb = _lib.CavoidPolicyTrainBuffers()
    lb.struct_size = C.sizeof(_lib.CavoidPolicyTrainBuffers)
    x = torch.zeros((65, ws20.input_size), device="cuda")
    y, a = torch.zeros(65, device="cuda"), torch.zeros(65, dtype=torch.int32, device="cuda")
    assert lib.cavoid_policy_train(hd, p(x), 64, ws20.input_size, p(y), p(a), 1e-4, 1e-6, C.byref(lb), None) == -1
    _, good = tr._scratch(64)
    bad = _lib.CavoidPolicyTrainWsBuffers.from_buffer_copy(good)
    bad.struct_size = C.sizeof(_lib.CavoidPolicyTrainWsBuffers) - 8
    assert lib.cavoid_policy_train_ws(hd, p(x), 64, ws20.input_size, p(y), p(a), 1e-4, 1e-6, C.byref(bad), None) == -1
    assert lib.cavoid_policy_train_ws(hd, p(x), 65, ws20.input_size, p(y), p(a), 1e-4, 1e-6, C.byref(good), None) == -1     # capacity_rows < rows
    assert lib.cavoid_policy_train_ws(hd, p(x), 64, ws20.input_size - 1, p(y), p(a), 1e-4, 1e-6, C.byref(good), None) == -1  # stride < row
    assert lib.cavoid_policy_train_ws(hd, p(x), 64, ws20.input_size, p(y), p(a), 1e-4, 1e-6, C.byref(good), None) == 0
    assert lib.cavoid_policy_train_regression_ws(hd, p(x), 64, ws20.input_size, p(y), p(a), C.byref(good), None) == 0
    torch.cuda.synchronize()
