"""The fused policy on crowd rows (20..64 observed agents): policy_crowd_forward_kernel (cavoid_policy_crowd.hpp) against the PyTorch
graph and float64, bit for bit the default kernel on narrow rows, its launch contract (row list, strided rows, hipGraph), and the layers
above it -- BatchedRollout, evaluate, the training CLI -- in crowd worlds."""
import copy
import ctypes as C

import pytest
import torch

from tests.gpu_support import _env
from tests.policy_support import P_TOL, V_TOL, _inputs, _net

pytestmark = pytest.mark.gpu

RING = 23                                                   # kSpCrowdRing: agent t sits in slot 1 + t % 23
CROWD = ("CROWD", 0)


def _mixed_lengths(x, M, seed, fractional=False):
    """per-row lengths 0 .. M mixed inside every tile, and (when there are enough rows) whole tiles of full rows.  `fractional`: some counts
    x.5 -- the kernels' own rule for those (a step past floor is live only when another row of the tile runs it) is not the PyTorch graph's,
    so only the kernel-against-kernel tests use them"""
    B = x.shape[0]
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(0, M + 1, (B,), generator=g).to(torch.float32)
    if fractional:
        n[torch.arange(B) % 7 == 3] += 0.5
    n = n.clamp(max=float(M))
    if B >= 256:
        n[64:192] = float(M)                                 # two tiles where every row is full (the ALL_LIVE path)
    x[:, 0] = n.cuda()
    return x


@pytest.mark.parametrize("M", [20, RING, RING + 1, 31, 47, 63, 64])
@pytest.mark.parametrize("B", [1, 63, 64, 130, 8192])
def test_crowd_forward_matches_torch_fp32(M, B):
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    net = _net(M, seed=M)
    pol = FusedPolicy(net)
    assert pol.crowd and pol.inference_form == ("split", 16)
    x = _mixed_lengths(_inputs(net, B, seed=B + M), M, seed=M)
    p, v = pol(x)
    with torch.no_grad():
        _, p_ref, v_ref = net.forward(x)
    assert (p - p_ref).abs().max().item() <= P_TOL
    assert ((v - v_ref).abs() <= V_TOL + V_TOL * v_ref.abs()).all()
    assert (p.sum(dim=1) - 1.0).abs().max().item() <= 1e-5


@pytest.mark.parametrize("kernel", ["f16", "split3"])
def test_crowd_kernel_against_a_float64_yardstick(kernel, monkeypatch):
    """test_gpu_policy.py's float64 bars after up to 63 LSTM steps: the float16 form is held to float32 grade (absolute, or -- where the
    absolute bar fails -- within 6x of the float32 PyTorch graph's own error), the bf16 form to a quarter of P_TOL / V_TOL."""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    monkeypatch.setenv("CAVOID_POLICY_PRODUCTS", "16" if kernel == "f16" else "3")
    for M, B, scale in ((31, 4096, 1.0), (63, 2048, 1.0), (31, 4096, 4.0), (63, 2048, 4.0)):
        net = _net(M, seed=40 + M)
        pol = FusedPolicy(net)
        assert pol.inference_form == ("split", 16 if kernel == "f16" else 3)
        x = _inputs(net, B, seed=7, scale=scale)
        p, v = pol(x)
        with torch.no_grad():
            _, p32, v32 = net.forward(x)
            _, p64, v64 = copy.deepcopy(net).double().forward(x.double())
        e_kernel_p, e_torch_p = (p.double() - p64).abs().max().item(), (p32.double() - p64).abs().max().item()
        e_kernel_v, e_torch_v = (v.double() - v64).abs().max().item(), (v32.double() - v64).abs().max().item()
        print("crowd policy kernel %s M=%d scale=%g: |dp| %.2e (torch f32 %.2e)  |dv| %.2e (torch f32 %.2e)"
              % (kernel, M, scale, e_kernel_p, e_torch_p, e_kernel_v, e_torch_v))
        info = (kernel, M, scale, e_kernel_p, e_torch_p, e_kernel_v, e_torch_v)
        assert e_kernel_p <= P_TOL and e_kernel_v <= V_TOL * (1.0 + v64.abs().max().item()), info
        if kernel == "f16":
            absolute = e_kernel_p <= 1e-6 and e_kernel_v <= 5e-6
            relative = e_kernel_p <= 6.0 * e_torch_p + 5e-8 and e_kernel_v <= 6.0 * e_torch_v + 5e-7
            assert absolute or relative, info
        else:
            assert e_kernel_p <= P_TOL / 4 and e_kernel_v <= V_TOL / 4 * (1.0 + v64.abs().max().item()), info


def _narrow_and_wide(seed):
    """one network's parameters in an M = 19 and an M = 63 network (no weight shape depends on M), the normalisation of the first 19 agents
    shared"""
    narrow, wide = _net(19, seed=seed), _net(63, seed=seed)
    with torch.no_grad():
        for name, prm in narrow.named_parameters():
            getattr(wide, name).copy_(prm)
        wide.avg[:narrow.input_size].copy_(narrow.avg)
        wide.std[:narrow.input_size].copy_(narrow.std)
    return narrow, wide


@pytest.mark.parametrize("B", [4096, 131072])                # quad / duo form of the M = 19 handle (duo from 2 tiles per CU)
def test_crowd_kernel_is_bitwise_the_default_kernel_on_narrow_rows(B):
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    narrow, wide = _narrow_and_wide(seed=5)
    x19 = _mixed_lengths(_inputs(narrow, B, seed=3), 19, seed=4, fractional=True)
    x63 = torch.zeros((B, wide.input_size), device="cuda")
    x63[:, :narrow.input_size] = x19
    pn, pw = FusedPolicy(narrow, seed=9), FusedPolicy(wide, seed=9)
    assert not pn.crowd and pw.crowd
    for greedy in (True, False):
        an, p_n, v_n = pn.act(x19, greedy=greedy)
        aw, p_w, v_w = pw.act(x63, greedy=greedy)
        assert torch.equal(p_n, p_w) and torch.equal(v_n, v_w) and torch.equal(an, aw), greedy


def test_crowd_row_list_equals_the_full_pass_on_the_listed_rows():
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    net = _net(47, seed=51)
    B = 5000
    x = _mixed_lengths(_inputs(net, B, seed=6), 47, seed=2)      # (integer counts: a row list regroups rows into other tiles)
    g = torch.Generator().manual_seed(1)
    listed = torch.randperm(B, generator=g)[:3210].to(torch.int32).cuda()
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


def test_crowd_policy_runs_on_the_env_observation_tensor_in_place():
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    W, N = 32, 64
    env = _env(W, N, seed=4, gen_pool_size=0, gen_min_agents=2)
    obs = env.reset()
    for _ in range(3):
        obs = env.step(torch.randint(0, 11, (W, N), dtype=torch.int32, device="cuda"))[0]
    net = NetworkVP_rnn(env.config).to("cuda:0")
    pol = FusedPolicy(net, seed=3)
    x = obs.view(W * N, -1)[:, 1:]
    assert x.stride(0) == env.obs_width and not x.is_contiguous()
    a1, p1, v1 = pol.act(x)
    pol.seed(3)
    a2, p2, v2 = pol.act(x.contiguous())
    assert torch.equal(a1, a2) and torch.equal(p1, p2) and torch.equal(v1, v2)
    env.close()


def test_crowd_policy_in_a_hip_graph():
    """a captured act replayed K times = K eager calls: the launch counter lives on the device and advances per launch"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    net = _net(63, seed=8)
    x = _mixed_lengths(_inputs(net, 3000, seed=8), 63, seed=8)
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


def _crowd_rollout(N, monkeypatch, frozen=False):
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    over = dict(gen_nonlearning_fraction=0.5, gen_static_fraction=0.3, gen_rvo_fraction=0.0, gen_frozen_fraction=0.6) if frozen else {}
    env = _env(64, N, seed=2, gen_pool_size=0, gen_min_agents=2, **over)
    net = NetworkVP_rnn(env.config).to("cuda:0")
    pol = FusedPolicy(net, seed=3)
    frozen_pol = FusedPolicy(copy.deepcopy(net), seed=0) if frozen else None

    def no_torch_network(*a, **k):
        raise AssertionError("the PyTorch network ran")
    monkeypatch.setattr(NetworkVP_rnn, "predict_p_and_v", no_torch_network)
    roll = BatchedRollout(env, pol, time_max=3, frozen_policy=frozen_pol)
    assert not roll.fused_available and "more than 16 agents" in roll.fused_unavailable_reason
    roll.reset()
    for _ in range(12):
        roll.step()
    assert env.last_step_form == CROWD
    assert torch.isfinite(env.obs).all()
    if env.obs_width - 1 <= 255:
        # (cavoid_rollout_compact copies training rows of at most 255 floats: a 64-agent row has 446, its drain is CAVOID_EUNSUPPORTED)
        batch = roll.drain()
        assert len(batch) > 0 and batch.x.shape[1] == env.obs_width - 1
        assert torch.isfinite(batch.x).all() and torch.isfinite(batch.r).all()
        assert int(batch.a_index.min()) >= 0 and int(batch.a_index.max()) < net.num_actions
    roll.close(); env.close()


@pytest.mark.parametrize("N", [32, 64])
def test_crowd_rollout_acts_on_the_fused_policy(N, monkeypatch):
    _crowd_rollout(N, monkeypatch)


def test_crowd_rollout_with_frozen_network_agents(monkeypatch):
    _crowd_rollout(32, monkeypatch, frozen=True)


def test_evaluate_on_crowd_worlds_with_the_fused_policy():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    env = _env(64, 32, seed=6, gen_pool_size=0, gen_min_agents=2, evaluate_mode=1)
    pol = FusedPolicy(NetworkVP_rnn(env.config).to("cuda:0"), seed=1)
    r = evaluate(env, pol, rounds=1, max_steps=80)
    assert r["agents"] > 0 and r["env_steps"] > 0
    assert abs(r["success_rate"] + r["collision_rate"] + r["timeout_rate"] + r["unfinished_rate"] - 1.0) < 1e-9
    assert all(0.0 <= r[k] <= 1.0 for k in ("success_rate", "collision_rate", "timeout_rate", "unfinished_rate"))
    env.close()


def test_what_crowd_handles_refuse(monkeypatch):
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer, FusedPolicy
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    with pytest.raises(ValueError, match="19"):
        FusedA3CTrainer(_net(20, seed=1))
    with monkeypatch.context() as m:
        m.setenv("CAVOID_POLICY_F32", "1")
        with pytest.raises(_lib.CavoidError) as e:
            FusedPolicy(_net(31, seed=1))
        assert e.value.code == -4                            # CAVOID_EUNSUPPORTED
    # an env of 8 agents whose rows are padded to 30 observed agents: the fused actor kernel refuses, the step-by-step path runs
    env = _env(64, 8, 30, seed=3, gen_pool_size=0, gen_min_agents=2)
    pol = FusedPolicy(NetworkVP_rnn(env.config).to("cuda:0"), seed=2)
    roll = BatchedRollout(env, pol, time_max=3)
    assert not roll.fused_available and "observes 30 neighbours" in roll.fused_unavailable_reason
    roll.reset()
    b = roll._actor_buffers()
    p = BatchedCollisionAvoidanceEnv._ptr
    cur, nxt = roll._obs_buffers[roll._cur], roll._obs_buffers[1 - roll._cur]
    rc = roll._lib.cavoid_actor_run(env._h, pol._h, roll._h, C.byref(b), p(cur), p(nxt), p(env.rewards), p(env.done), p(env.game_over),
                                    p(roll._act_out), p(roll._val_out), 1, 0, env._stream())
    assert rc == -4                                          # CAVOID_EUNSUPPORTED
    for _ in range(6):
        roll.step()
    batch = roll.drain()
    assert len(batch) > 0 and torch.isfinite(batch.x).all()
    roll.close(); env.close()


def test_train_cli_on_crowd_worlds(tmp_path, capsys):
    import glob
    from rl_collision_avoidance_amd.ga3c import train
    ck = str(tmp_path / "ck")
    train.main(["--agents", "32", "--worlds", "64", "--episodes", "64", "--pretrain-steps", "0", "--print-every", "0",
                "--checkpoint-dir", ck, "--save-every", "32", "--train-rows", "2048"])
    out = capsys.readouterr().out
    assert "policy: the fused crowd policy kernel for acting, the autograd trainer" in out
    assert "finished" in out
    files = sorted(glob.glob(ck + "/network_*.pt"))
    assert files
    state = torch.load(files[-1], map_location="cpu")
    assert state["training_step"] > 0 and "lstm_kernel" in state["model"]
