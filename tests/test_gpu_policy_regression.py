"""The supervised start (train_regression_op on cost_regression, NetworkVPCore.py:90-100,123) on the fused trainer kernels:
cavoid_policy_train_regression / _ws, FusedA3CTrainer.train_regression, regression.pretrain(trainer=...) and ga3c.train.

The yardstick throughout is ``ga3c.regression.regression_loss`` under float64 autograd, never the kernels themselves; the criterion
is policy_regimes.assert_gradients_match / assert_loss_matches (no new tolerance).  tests/regression_regimes.py builds the cases and
tests/test_policy_regression_host.py holds them to their conditions on the CPU and shows what a wrong head would do to them."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

from tests import policy_regimes as R
from tests import regression_regimes as G

pytestmark = pytest.mark.gpu


def _regress_and_check(case, net, x, y, a, tr, x_kernel=None):
    cost_p, cost_v, want, torch32 = G.reference_gradients(net, x, y, a)
    got_p, got_v = tr.train_regression(x if x_kernel is None else x_kernel, y, a)
    assert got_p.device.type == "cuda" and got_p.dim() == 0 and got_v.dim() == 0
    got_p, got_v = float(got_p), float(got_v)
    report = []
    try:
        R.assert_loss_matches(got_p, cost_p)
        R.assert_loss_matches(got_v, cost_v)
        R.assert_gradients_match(net, want, torch32, case.B, report)
    finally:
        print("%s: cost_p %.6e (float64 %.6e)  cost_v %.6e (float64 %.6e)" % (G.case_id(case), got_p, cost_p, got_v, cost_v))
        for k, err, err32, scale in report:
            print("    %-14s err %.2e  err32 %.2e  scale %.2e  err/scale %.1e" % (k, err, err32, scale, err / scale))
    return want


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_regression_head_matches_float64_autograd(case):
    """cavoid_policy_train_regression / _ws + the weight-gradient GEMMs, learning rate 0: every gradient and both loss sums"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    net, x, y, a, info = G.build_case(case, "cuda")
    G.assert_conditions(case, info)
    tr = FusedA3CTrainer(net, learning_rate=0.0)
    assert tr.ws == (case.arch == "weight_sharing")
    before = {k: t.detach().clone() for k, t in net.named_parameters()}
    _regress_and_check(case, net, x, y, a, tr)
    assert tr.training_step == 0 and tr.frame_counter == 0          # (RL steps only)
    assert all(torch.equal(t, before[k]) for k, t in net.named_parameters())


@pytest.mark.parametrize("arch,M", [("rnn", 3), ("weight_sharing", 7)])
@pytest.mark.parametrize("A", [5, 15])
def test_other_action_counts(arch, M, A):
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    case = G.Case("fresh", arch, M, 777, 0.0, 0.0, A)
    net, x, y, a, info = G.build_case(case, "cuda")
    G.assert_conditions(case, info)
    assert int(a.max()) == A - 1
    _regress_and_check(case, net, x, y, a, FusedA3CTrainer(net, learning_rate=0.0))


@pytest.mark.parametrize("arch,M", [("rnn", 9), ("weight_sharing", 3)])
def test_rows_as_a_strided_view(arch, M):
    """x as the env hands it over: a column slice (obs[:, 1:]) of wider rows, not copied"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    case = G.Case("fresh", arch, M, 1000, 0.0, 0.0, 11)
    net, x, y, a, _ = G.build_case(case, "cuda")
    obs = torch.full((case.B, net.input_size + 3), float("nan"), device="cuda")
    obs[:, 1:1 + net.input_size] = x
    view = obs[:, 1:1 + net.input_size]
    assert not view.is_contiguous()
    _regress_and_check(case, net, x, y, a, FusedA3CTrainer(net, learning_rate=0.0), x_kernel=view)


@pytest.mark.parametrize("arch,M", [("rnn", 9), ("weight_sharing", 7)])
def test_regression_writes_every_scratch_row_it_lets_the_gemms_read(arch, M):
    """test_trainer_writes_every_scratch_row_it_lets_the_gemms_read for the regression launch pair: NaN-filled scratch, a batch that
    ends inside a 2048-row slice and holds a tile whose rows all stop after one LSTM step"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    B = 2100
    case = G.Case("fresh", arch, M, B, 0.0, 0.0, 11)
    net = R.build_net(arch, M, seed=G.NET_SEED).cuda()
    x = R.inputs(net, 3200, seed=B + 1)
    x = x[R.clear_of_relu_kinks(net, x)]
    short = x[:, 0] <= 1.0
    x = torch.cat([x[~short][:64], x[short][:64], x[~short][64:]])[:B]
    assert x.shape[0] == B and float(x[64:128, 0].max()) == 1.0 and float(x[:, 0].max()) == M
    g = torch.Generator().manual_seed(B)
    y, a = torch.randn(B, generator=g).cuda(), torch.randint(0, 11, (B,), generator=g).cuda()
    tr = FusedA3CTrainer(net, learning_rate=0.0)
    buffers, _ = tr._scratch(4096)
    for t in buffers.values():
        t.fill_(float("nan"))
    _regress_and_check(case, net, x, y, a, tr)
    assert tr._scratch(4096)[0] is buffers and len(tr._buffers) == 1
    assert float(buffers["gh"][B:].abs().max()) == 0.0                # rows past `rows`: zero gradient


@pytest.mark.parametrize("arch,M", [("rnn", 3), ("weight_sharing", 3)])
def test_no_rows(arch, M):
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    net = R.build_net(arch, M, seed=41).cuda()
    tr = FusedA3CTrainer(net)
    before = {k: t.detach().clone() for k, t in net.named_parameters()}
    x = R.inputs(net, 128, seed=5)
    cost_p, cost_v = tr.train_regression(x[:0], torch.zeros(0).cuda(), torch.zeros(0, dtype=torch.int64).cuda())
    assert float(cost_p) == 0.0 and float(cost_v) == 0.0 and tr.training_step == 0
    assert all(torch.equal(t, before[k]) for k, t in net.named_parameters())


def _leak_check(arch, M, rows_regression, rows_a3c):
    """train_regression() on the first rows_regression rows, then train() on the first rows_a3c rows on the same trainer (both
    batches round up to the same scratch); a fresh trainer runs the A3C step alone.  -> ({name: the fresh trainer's gradient},
    {name: the used trainer's}, the A3C step's (net, x, y, a) with the used trainer's gradients in net)"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    case = G.Case("gain40", arch, M, 1000, 0.0, R.GAIN_TRAINER, 11)
    net, x, y, a, _ = G.build_case(case, "cuda")
    clear = R.clear_of_threshold(net, x, net.log_epsilon)              # (the A3C head's clamp: policy_regimes.build_case's row filter)
    assert 1.0 - clear.float().mean().item() <= R.MAX_EXCLUDED
    x, y, a = x[clear], y[clear], a[clear]
    g = torch.Generator().manual_seed(99)
    y2, a2 = torch.randn(x.shape[0], generator=g).cuda(), torch.randint(0, 11, (x.shape[0],), generator=g).cuda()
    fresh = FusedA3CTrainer(net, learning_rate=0.0)
    fresh.train(x[:rows_a3c], y2[:rows_a3c], a2[:rows_a3c])
    want = {k: t.grad.clone() for k, t in net.named_parameters()}
    used = FusedA3CTrainer(net, learning_rate=0.0)
    used.train_regression(x[:rows_regression], y[:rows_regression], a[:rows_regression])
    moved = [k for k, t in net.named_parameters() if not torch.equal(t.grad, want[k])]
    assert "p_kernel" in moved and "v_kernel" in moved                 # (the regression gradients are other gradients)
    used.train(x[:rows_a3c], y2[:rows_a3c], a2[:rows_a3c])
    assert len(used._buffers) == 1 and len(fresh._buffers) == 1 and list(used._buffers) == list(fresh._buffers)
    return want, {k: t.grad.clone() for k, t in net.named_parameters()}, (net, x[:rows_a3c], y2[:rows_a3c], a2[:rows_a3c])


@pytest.mark.parametrize("arch,M", R.ARCH_M)
def test_a3c_step_after_a_regression_step_is_a_fresh_trainers(arch, M):
    """Nothing leaks through the scratch buffers: train() after train_regression() on the same trainer leaves EVERY gradient
    bitwise equal to a fresh trainer's on the same weights.  The regression step fills all 64 rows of the scratch, the A3C step
    then has 16: the one-wavefront batch is the size at which a fresh trainer's own gradients are reproducible bit for bit -- the
    kernels sum the bias gradients with float atomics, one per wavefront and column, so with more rows the order of those
    additions, and with it the last bits of the six bias gradients, changes from launch to launch (measured at 1000 rows, where a
    used and a fresh trainer agree bitwise in every weight gradient: lstm_bias / other_bias 3.8e-6 .. 4.6e-5, layer1_bias 3.8e-6 ..
    1.5e-5, layer2_bias 7.6e-6 .. 4.6e-5, fc1_bias 7.6e-6 .. 4.6e-5, v_bias 1.9e-6 .. 1.5e-5, p_bias 7.2e-7 .. 5.7e-6 apart, the size
    of one rounding of such a sum; test_..._at_1000_rows holds the weight gradients there)."""
    want, got, _ = _leak_check(arch, M, 64, 16)
    differ = {k: (got[k] - want[k]).abs().max().item() for k in want if not torch.equal(got[k], want[k])}
    print("%s M=%d, 64 then 16 rows: gradients that differ from the fresh trainer's: %s" % (arch, M, differ or "none"))
    assert not differ, differ


@pytest.mark.parametrize("arch,M", R.ARCH_M)
def test_a3c_step_after_a_regression_step_is_a_fresh_trainers_at_1000_rows(arch, M):
    """the same on 1000 rows (16 workgroups): every weight gradient -- the GEMMs over what the launch pair left in the scratch --
    is bitwise the fresh trainer's.  The bias gradients are summed with float atomics across workgroups, in an order that changes from
    launch to launch: they, with every other gradient of the used trainer, are held to float64 autograd of NetworkVP_rnn.loss under
    policy_regimes.assert_gradients_match, the criterion of the A3C pass's own tests"""
    want, got, (net, x, y, a) = _leak_check(arch, M, 1000, 1000)
    differ = {k: (got[k] - want[k]).abs().max().item() for k in want if not torch.equal(got[k], want[k])}
    print("%s M=%d, 1000 rows: gradients that differ from the fresh trainer's: %s" % (arch, M, differ or "none"))
    assert not [k for k in differ if not k.endswith("_bias")], differ
    _, _, _, want64, torch32 = R.reference_gradients(net, x, y, a)       # (clears net's .grad)
    for k, t in net.named_parameters():
        t.grad = got[k]
    R.assert_gradients_match(net, want64, torch32, x.shape[0])


def test_abi_refusals():
    """the A3C pair's error codes: the other kind of handle, a wrong struct_size, a handle loaded without with_backward"""
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer, FusedPolicy
    lstm, ws = FusedPolicy(R.build_net("rnn", 3, seed=1).cuda()), FusedPolicy(R.build_net("weight_sharing", 3, seed=1).cuda())
    p = lambda t: C.c_void_p(t.data_ptr())
    x = torch.zeros((64, lstm.input_size), device="cuda")
    y, a = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda")
    lib = lstm._lib
    b, bw = _lib.CavoidPolicyTrainBuffers(), _lib.CavoidPolicyTrainWsBuffers()
    b.struct_size, bw.struct_size = C.sizeof(_lib.CavoidPolicyTrainBuffers), C.sizeof(_lib.CavoidPolicyTrainWsBuffers)
    assert lib.cavoid_policy_train_regression(ws._h, p(x), 64, lstm.input_size, p(y), p(a), C.byref(b), None) == -1
    assert lib.cavoid_policy_train_regression_ws(lstm._h, p(x), 64, lstm.input_size, p(y), p(a), C.byref(bw), None) == -1
    # (without with_backward: what the A3C calls return)
    for pol, new, old, buf in ((lstm, lib.cavoid_policy_train_regression, lib.cavoid_policy_train, b),
                               (ws, lib.cavoid_policy_train_regression_ws, lib.cavoid_policy_train_ws, bw)):
        want = old(pol._h, p(x), 64, pol.input_size, p(y), p(a), 1e-4, 1e-6, C.byref(buf), None)
        assert want == -1 and new(pol._h, p(x), 64, pol.input_size, p(y), p(a), C.byref(buf), None) == want
    # a wrong struct_size on handles that could train: an error code, not a crash
    for net_arch, new, struct in (("rnn", lib.cavoid_policy_train_regression, _lib.CavoidPolicyTrainBuffers),
                                  ("weight_sharing", lib.cavoid_policy_train_regression_ws, _lib.CavoidPolicyTrainWsBuffers)):
        tr = FusedA3CTrainer(R.build_net(net_arch, 3, seed=1).cuda())
        _, good = tr._scratch(64)
        bad = struct.from_buffer_copy(good)
        bad.struct_size = C.sizeof(struct) - 8
        assert new(tr.policy._h, p(x), 64, tr.policy.input_size, p(y), p(a), C.byref(bad), None) == -1
        assert new(tr.policy._h, p(x), 64, tr.policy.input_size, p(y), p(a), C.byref(good), None) == 0
        assert new(tr.policy._h, p(x), 65, tr.policy.input_size, p(y), p(a), C.byref(good), None) == -1     # capacity_rows < rows
    torch.cuda.synchronize()


@pytest.mark.parametrize("arch", ["rnn", "weight_sharing"])
def test_pretraining_on_the_fused_trainer_clones_the_teacher(arch, monkeypatch):
    """test_regression_pretraining_clones_the_teacher's run and bounds with trainer=FusedA3CTrainer(net); the PyTorch loss functions
    raise during the run, and the trainer's FusedPolicy then acts as the regressed network does (the packed weights were refreshed)"""
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.ga3c import regression
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    env = BatchedCollisionAvoidanceEnv(512, seed=4)
    net = R.build_net(arch, 3, seed=71).cuda()
    tr = FusedA3CTrainer(net)
    before = {k: t.detach().clone() for k, t in net.named_parameters()}

    def no_pytorch_loss(*args, **kwargs):
        raise AssertionError("the PyTorch loss ran")
    with monkeypatch.context() as mp:
        mp.setattr(NetworkVP_rnn, "loss", no_pytorch_loss)
        mp.setattr(regression, "regression_loss", no_pytorch_loss)
        info = regression.pretrain(net, env, steps=60, learning_rate=2e-3, rows_per_step=8192, trainer=tr)
    print("%s: %s" % (arch, info))
    assert sorted(info) == ["p_loss_per_row", "steps", "teacher_episode_reward", "v_loss_per_row"]
    assert info["steps"] == 60 and info["p_loss_per_row"] < 0.2
    assert tr.training_step == 0 and not any(torch.equal(t, before[k]) for k, t in net.named_parameters())
    obs = env.reset()
    table = torch.as_tensor(__import__("rl_collision_avoidance_amd.actions", fromlist=["Actions"]).Actions().actions,
                            dtype=torch.float32, device="cuda")
    with torch.no_grad():
        _, p, _ = net.forward(obs.view(512 * 4, -1)[:, 1:].contiguous())
    agree = (p.argmax(dim=1).view(512, 4) == regression.teacher_actions(obs, table).long()).float().mean().item()
    assert agree > 0.9
    greedy, _, _ = tr.policy.act(obs.view(512 * 4, -1)[:, 1:], greedy=True)
    same = (greedy.long() == p.argmax(dim=1)).float().mean().item()
    print("%s: argmax agreement with the teacher %.4f, fused greedy actions equal to the network's argmax on %.4f of the rows" % (arch, agree, same))
    assert same >= 0.999                                               # (a near-tie of two probabilities may fall either way)
    env.close()


CLI = ["--agents", "4", "--worlds", "256", "--episodes", "100", "--print-every", "0", "--train-rows", "4096", "--pretrain-steps", "20"]


# (the fused path is opt-in, --fused-regression, as long as profiles/policy_regression_timing.txt holds no measurement that shows it
#  no slower than the autograd step: the rule the default follows)
@pytest.mark.parametrize("extra,line", [(["--fused-regression"], "[Regression] on the fused rnn trainer kernels"),
                                        (["--fused-regression", "--arch", "weight_sharing", "--observed", "7"],
                                         "[Regression] on the fused weight_sharing trainer kernels"),
                                        (["--fused-regression", "--autograd-trainer"], "[Regression] through PyTorch autograd"),
                                        (["--autograd-trainer"], "[Regression] through PyTorch autograd"),
                                        ([], "[Regression] through PyTorch autograd (the default until the fused rnn trainer kernels are timed")])
def test_train_cli_names_the_regression_path(extra, line, capsys):
    from rl_collision_avoidance_amd.ga3c import train
    train.main(CLI + extra)
    out = capsys.readouterr().out
    assert line in out and out.count("[Regression] on") + out.count("[Regression] through") == 1
    assert "[Regression] done" in out and "finished" in out
