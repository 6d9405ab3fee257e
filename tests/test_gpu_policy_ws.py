"""The weight-sharing network (MULTI_AGENT_ARCH 'weight_sharing') on its fused HIP kernels (cavoid_policy_ws.hpp, through
cavoid_policy_*_ws): inference against the PyTorch float32 graph and float64, the action draw, the launch contract (row list, strided
rows, hipGraph), the trainer pass against float64 autograd and the autograd trainer, and the layers above it -- BatchedRollout (also
with frozen-network agents), the refusals of the fused actor kernel, and the training CLI."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.cavoid_oracle import philox4x32
from tests.policy_regimes import assert_gradients_match
from tests.gpu_support import _env
from tests.policy_support import P_TOL, V_TOL, _inputs

pytestmark = pytest.mark.gpu


def _ws_net(M, seed=0, min_policy=0.0, normalize=True, A=11):
    from rl_collision_avoidance_amd.config import EnvConfig
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = M + 1
            EnvConfig.__init__(self)
    cfg = Cfg()
    cfg.MIN_POLICY = min_policy
    cfg.NORMALIZE_INPUT = normalize
    net = NetworkVP_rnn(cfg, num_actions=A, seed=seed, arch="weight_sharing").cuda()
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():                      # non-zero biases: every bias path (other_bias too) is exercised
        for name, prm in net.named_parameters():
            if name.endswith("_bias"):
                prm.copy_((torch.rand(prm.shape, generator=g) - 0.5).to(prm.device))
    return net


def _check(p, v, p_ref, v_ref):
    assert torch.isfinite(p).all() and torch.isfinite(v).all()
    assert (p - p_ref).abs().max().item() <= P_TOL
    assert ((v - v_ref).abs() <= V_TOL + V_TOL * v_ref.abs()).all()


@pytest.mark.parametrize("M", [1, 3, 5, 7, 19])
@pytest.mark.parametrize("B", [1, 63, 64, 130, 32768])
def test_ws_forward_matches_torch_fp32(M, B):
    """counts drawn over 0..M; _inputs fills every slot with random values, also past the row's count: no early exit"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    net = _ws_net(M, seed=M)
    pol = FusedPolicy(net)
    assert pol.inference_form == ("f32", 0)
    x = _inputs(net, B, seed=B)
    p, v = pol(x)
    with torch.no_grad():
        _, p_ref, v_ref = net.forward(x)
    assert p.shape == (B, 11) and v.shape == (B,)
    _check(p, v, p_ref, v_ref)
    assert (p.sum(dim=1) - 1.0).abs().max().item() <= 1e-5


@pytest.mark.parametrize("min_policy,normalize", [(1e-3, True), (1e-3, False)])
def test_ws_min_policy_and_unnormalised_input(min_policy, normalize):
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    net = _ws_net(7, seed=5, min_policy=min_policy, normalize=normalize)
    pol = FusedPolicy(net)
    x = _inputs(net, 777, seed=1, scale=0.3 if not normalize else 1.0)
    p, v = pol(x)
    with torch.no_grad():
        _, p_ref, v_ref = net.forward(x)
    _check(p, v, p_ref, v_ref)


def test_ws_padded_slots_go_through_the_filter():
    """the slots past a row's count still feed layer1 (is_on = 0, the normalised values and the bias): changing them changes p"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    net = _ws_net(5, seed=12)
    pol = FusedPolicy(net)
    x = _inputs(net, 256, seed=3)
    x[:, 0] = 2.0
    p0, _ = pol(x)
    x2 = x.clone()
    x2[:, 1 + 4 + 7 * 3:] += 1.0                               # slots 3 and 4: past every row's count
    p1, v1 = pol(x2)
    with torch.no_grad():
        _, p_ref, v_ref = net.forward(x2)
    _check(p1, v1, p_ref, v_ref)
    assert not torch.allclose(p0, p1)


@pytest.mark.parametrize("M", [3, 7])
def test_ws_kernel_against_a_float64_yardstick(M):
    """float32-MFMA products are exact: the bar of test_both_inference_kernels_against_a_float64_yardstick, also at x4 inputs"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    for scale in (1.0, 4.0):
        net = _ws_net(M, seed=40 + M)
        pol = FusedPolicy(net)
        x = _inputs(net, 4096, seed=7, scale=scale)
        p, v = pol(x)
        with torch.no_grad():
            _, p32, v32 = net.forward(x)
            _, p64, v64 = copy.deepcopy(net).double().forward(x.double())
        e_p, e_torch_p = (p.double() - p64).abs().max().item(), (p32.double() - p64).abs().max().item()
        e_v, e_torch_v = (v.double() - v64).abs().max().item(), (v32.double() - v64).abs().max().item()
        print("ws policy kernel M=%d scale=%g: |dp| %.2e (torch f32 %.2e)  |dv| %.2e (torch f32 %.2e)" % (M, scale, e_p, e_torch_p, e_v, e_torch_v))
        assert e_p <= 1e-6 and e_v <= 5e-6, (M, scale, e_p, e_torch_p, e_v, e_torch_v)


def test_ws_greedy_is_argmax_and_sampling_is_the_inverse_cdf():
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    net = _ws_net(7, seed=7)
    SEED = 0x1234567890AB
    pol = FusedPolicy(net, seed=SEED)
    B = 5000
    x = _inputs(net, B, seed=8)
    a_g, p, _ = pol.act(x, greedy=True)
    assert torch.equal(a_g.long(), p.argmax(dim=1))
    draws = []
    for _ in range(3):
        a, p, _ = pol.act(x)
        draws.append(a.cpu().numpy())
    cdf = np.cumsum(p.cpu().numpy().astype(np.float64), axis=1)
    for k, a in enumerate(draws):
        step, bad = 1 + k, 0
        for row in range(0, B, 7):
            bits = philox4x32(row, 0, step, 0x504F4C, SEED & 0xFFFFFFFF, SEED >> 32)[0]
            u = (bits >> 8) / 16777216.0
            expect = min(int(np.sum(cdf[row] <= u * cdf[row, -1])), 10)
            if expect != a[row]:
                assert np.min(np.abs(cdf[row] - u * cdf[row, -1])) < 1e-6, (row, step, expect, a[row])
                bad += 1
        assert bad <= 2
    assert not np.array_equal(draws[0], draws[1])
    pol.seed(SEED)
    pol.act(x, greedy=True)
    again, _, _ = pol.act(x)
    assert np.array_equal(again.cpu().numpy(), draws[0])


def test_ws_row_list_pass_equals_the_full_pass_on_the_listed_rows():
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    net = _ws_net(5, seed=51)
    B = 5000
    x = _inputs(net, B, seed=6)
    listed = torch.randperm(B, generator=torch.Generator().manual_seed(1))[:3210].to(torch.int32).cuda()
    index = torch.zeros(B, dtype=torch.int32, device="cuda")
    index[:listed.numel()] = listed
    count = torch.tensor([listed.numel()], dtype=torch.int32, device="cuda")
    pol = FusedPolicy(net, seed=77)
    a_full, p_full, v_full = pol.act(x)
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


def test_ws_policy_in_a_hip_graph():
    """a captured act replayed K times = K eager calls: the launch counter lives on the device and advances per launch"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    net = _ws_net(7, seed=8)
    x = _inputs(net, 3000, seed=8)
    eager = FusedPolicy(net, seed=21)
    want = [eager.act(x)[0].clone() for _ in range(4)]
    pol = FusedPolicy(net, seed=21)
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            a, _, _ = pol.act(x)
    torch.cuda.synchronize()
    for k in range(4):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(a, want[k]), k
    assert not torch.equal(want[0], want[1])


def test_ws_policy_runs_on_the_env_observation_tensor_in_place():
    """4 agents observing M = 7 (the WS-8 shape: padded rows), closest_first; the obs tensor read through its row stride"""
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    W, N = 300, 4
    env = _env(W, N, 7, seed=3, gen_min_agents=2)
    obs = env.reset()
    for _ in range(20):
        obs = env.step_autoreset(torch.randint(0, 11, (W, N), dtype=torch.int32, device="cuda"))[0]
    net = NetworkVP_rnn(env.config, arch="weight_sharing").cuda()
    pol = FusedPolicy(net, seed=3)
    view = obs.view(W * N, -1)[:, 1:]
    assert not view.is_contiguous() and view.shape[1] == net.input_size
    assert len(torch.unique(view[:, 0])) >= 2
    p, v = pol(view)
    with torch.no_grad():
        _, p_ref, v_ref = net.forward(view.contiguous())
    _check(p, v, p_ref, v_ref)
    env.close()


@pytest.mark.parametrize("M", [3, 7, 19])
@pytest.mark.parametrize("B", [64, 1000, 32768])
def test_ws_fused_trainer_gradients_match_autograd(M, B):
    """cavoid_policy_train_ws + the weight-gradient GEMMs vs float64 autograd, under test_fused_trainer_gradients_match_autograd's criteria"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    net = _ws_net(M, seed=20 + M)
    x = _inputs(net, B, seed=B + 1)
    g = torch.Generator().manual_seed(B)
    y = torch.randn(B, generator=g).cuda()
    a = torch.randint(0, 11, (B,), generator=g).cuda()
    onehot = torch.nn.functional.one_hot(a, 11).float()
    ref_net = copy.deepcopy(net).double()
    total, _, _ = ref_net.loss(x.double(), y.double(), onehot.double())
    total.backward()
    want = {k: v.grad.clone() for k, v in ref_net.named_parameters()}
    net.zero_grad()
    net.loss(x, y, onehot)[0].backward()
    torch32 = {k: v.grad.clone() for k, v in net.named_parameters()}
    tr = FusedA3CTrainer(net, learning_rate=0.0)
    loss = float(tr.train(x, y, a))
    assert abs(loss - float(total.detach())) <= 2e-4 * max(1.0, abs(float(total.detach())))
    assert set(want) == {k for k, _ in net.named_parameters()} and "other_kernel" in want
    assert_gradients_match(net, want, torch32, B)          # (tests/policy_regimes.py: the one copy of the criterion)


def test_ws_fused_trainer_learns_like_the_autograd_trainer():
    from rl_collision_avoidance_amd.ga3c.network import A3CTrainer
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    net_a = _ws_net(7, seed=31)
    net_b = copy.deepcopy(net_a)
    ta, tb = A3CTrainer(net_a, learning_rate=1e-4), FusedA3CTrainer(net_b, learning_rate=1e-4)
    for step in range(5):
        x = _inputs(net_a, 4096, seed=100 + step)
        g = torch.Generator().manual_seed(step)
        y = torch.randn(4096, generator=g).cuda()
        a = torch.randint(0, 11, (4096,), generator=g).cuda()
        la = ta.train(x, y, torch.nn.functional.one_hot(a, 11).float())
        lb = float(tb.train(x, y, a))
        assert abs(la - lb) <= 1e-3 * max(1.0, abs(la))
    for (k, pa), (_, pb) in zip(net_a.named_parameters(), net_b.named_parameters()):
        d = (pa - pb).abs()
        # Adam moves an entry by ~lr per step whatever its gradient's size, so an entry whose gradient sums to the order of eps
        # (1e-8) over the batch turns float32 rounding of the two forward passes into a visible step: a handful of layer2 entries
        # (measured 6.4e-5 at most, lr = 1e-4).  Every other entry holds the 2e-5 bar of the LSTM network's test.
        assert (d > 2e-5).float().mean().item() <= 1e-3 and d.max().item() <= 1e-4, (k, d.max().item(), int((d > 2e-5).sum()))


def test_ws_fused_trainer_accepts_an_empty_batch():
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    net = _ws_net(7, seed=41)
    x = _inputs(net, 128, seed=5)
    tr = FusedA3CTrainer(net)
    loss = tr.train(x[:0], torch.zeros(0).cuda(), torch.zeros(0, dtype=torch.int64).cuda())
    assert float(loss) == 0.0 and tr.training_step == 1


def test_ws_limits_and_mixed_calls_are_refused():
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    with pytest.raises(ValueError, match="19"):
        FusedPolicy(_ws_net(20, seed=1))
    pol = FusedPolicy(_ws_net(3, seed=1))
    w = _lib.CavoidPolicyWeights()
    w.struct_size = C.sizeof(_lib.CavoidPolicyWeights)
    assert pol._lib.cavoid_policy_load(pol._h, C.byref(w), None) == -1              # an LSTM load on a WS handle: CAVOID_EINVAL
    b = _lib.CavoidPolicyTrainBuffers()
    b.struct_size = C.sizeof(_lib.CavoidPolicyTrainBuffers)
    x = torch.zeros((64, pol.input_size), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    assert pol._lib.cavoid_policy_train(pol._h, p(x), 64, pol.input_size, p(x), p(x), 0.0, 1e-6, C.byref(b), None) == -1
    use_split, products = C.c_int32(7), C.c_int32(7)
    assert pol._lib.cavoid_policy_info(pol._h, None, C.byref(use_split), C.byref(products), None) == 0
    assert use_split.value == 0 and products.value == 0


def _ws_rollout(monkeypatch, frozen):
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    over = dict(gen_nonlearning_fraction=0.5, gen_static_fraction=0.3, gen_rvo_fraction=0.0, gen_frozen_fraction=0.6) if frozen else {}
    env = _env(256, 4, 7, seed=2, gen_pool_size=0, gen_min_agents=2, **over)
    net = NetworkVP_rnn(env.config, arch="weight_sharing").cuda()
    pol = FusedPolicy(net, seed=3)
    frozen_pol = FusedPolicy(copy.deepcopy(net), seed=0) if frozen else None

    def no_torch_network(*a, **k):
        raise AssertionError("the PyTorch network ran")
    monkeypatch.setattr(NetworkVP_rnn, "predict_p_and_v", no_torch_network)
    roll = BatchedRollout(env, pol, frozen_policy=frozen_pol)
    assert not roll.fused_available and "weight_sharing" in roll.fused_unavailable_reason
    roll.reset()
    # the fused actor kernel refuses a weight-sharing handle, as policy and as frozen policy
    b = roll._actor_buffers()
    ptr = BatchedCollisionAvoidanceEnv._ptr
    cur, nxt = roll._obs_buffers[roll._cur], roll._obs_buffers[1 - roll._cur]
    args = (ptr(cur), ptr(nxt), ptr(env.rewards), ptr(env.done), ptr(env.game_over), ptr(roll._act_out), ptr(roll._val_out), 1, 0, env._stream())
    if frozen:
        assert roll._lib.cavoid_actor_run_mix(env._h, pol._h, frozen_pol._h, roll._h, C.byref(b), *args) == -4
    else:
        assert roll._lib.cavoid_actor_run(env._h, pol._h, roll._h, C.byref(b), *args) == -4
    if frozen:                                               # step by step (frozen rows: the frozen handle's row-list pass)
        for _ in range(32):
            roll.step()
    else:                                                    # the hipGraph form
        roll.capture(steps_per_graph=4)
        roll.replay(8)
    batch = roll.drain(flush_all=True)
    assert len(batch) > 1000 and batch.dropped == 0
    assert torch.isfinite(batch.x).all() and torch.isfinite(batch.r).all()
    assert int(batch.a_index.min()) >= 0 and int(batch.a_index.max()) < net.num_actions
    roll.close(); env.close()


def test_ws_rollout_acts_on_the_fused_policy(monkeypatch):
    _ws_rollout(monkeypatch, frozen=False)


def test_ws_rollout_with_frozen_network_agents(monkeypatch):
    _ws_rollout(monkeypatch, frozen=True)


def test_ws_train_cli_saves_resumes_evaluates_and_checks_the_arch(tmp_path, capsys):
    import glob
    from rl_collision_avoidance_amd.ga3c import train
    ck, ck_rnn = str(tmp_path / "ck"), str(tmp_path / "ck_rnn")
    base = ["--agents", "4", "--worlds", "256", "--print-every", "0", "--train-rows", "4096"]
    ws = ["--arch", "weight_sharing", "--observed", "7", "--sort-method", "closest_first"]
    train.main(base + ws + ["--episodes", "400", "--checkpoint-dir", ck, "--save-every", "200"])
    out = capsys.readouterr().out
    assert "the fused weight_sharing kernel for acting, the fused weight_sharing trainer kernels for training" in out
    assert "finished" in out and "training steps" in out and " 0 training steps" not in out
    files = sorted(glob.glob(ck + "/network_*.pt"))
    assert files
    state = torch.load(files[-1], map_location="cpu")
    assert state["arch"] == "weight_sharing" and state["max_others"] == 7
    assert "other_kernel" in state["model"] and "lstm_kernel" not in state["model"] and state["training_step"] > 0
    train.main(base + ws + ["--episodes", "100", "--load", files[-1]])
    assert "finished" in capsys.readouterr().out
    train.main(base + ws + ["--load", files[-1], "--evaluate", "1"])
    assert "[Evaluate]" in capsys.readouterr().out
    train.main(base + ["--episodes", "50", "--checkpoint-dir", ck_rnn])
    rnn_file = sorted(glob.glob(ck_rnn + "/network_*.pt"))[-1]
    capsys.readouterr()
    with pytest.raises(SystemExit, match="rnn network.*weight_sharing network"):
        train.main(base + ws + ["--episodes", "50", "--load", rnn_file])
