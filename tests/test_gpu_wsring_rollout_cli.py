"""The layers above the weight-sharing ring kernels: BatchedRollout acting on a ws-crowd FusedPolicy (24-agent worlds, 23 observed
neighbours), and ga3c.train --fused-crowd-ws -- acting, training and the supervised start on the ring kernels; without the flag, and with
a PyTorch switch beside it, every printed line stays what it was."""
import glob

import pytest

torch = pytest.importorskip("torch")

from tests.gpu_support import _env

pytestmark = pytest.mark.gpu

TODAY = "policy: the PyTorch network and the autograd trainer -- the fused weight_sharing kernels carry up to 19 observed neighbours, this run observes 23"


def test_rollout_acts_on_the_ws_crowd_policy(monkeypatch):
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    env = _env(64, 24, None, seed=2, gen_pool_size=0, gen_min_agents=2)
    net = NetworkVP_rnn(env.config, arch="weight_sharing").cuda()
    assert net.max_others == 23
    pol = FusedPolicy(net, seed=3, ws_crowd=True)
    assert pol.crowd and pol.ws

    def no_torch_network(*a, **k):
        raise AssertionError("the PyTorch network ran")
    monkeypatch.setattr(NetworkVP_rnn, "predict_p_and_v", no_torch_network)
    roll = BatchedRollout(env, pol)
    assert not roll.fused_available
    roll.reset()
    for _ in range(32):
        roll.step()
    batch = roll.drain(flush_all=True)
    assert len(batch) > 1000 and batch.dropped == 0
    assert batch.x.shape[1] == net.input_size
    assert torch.isfinite(batch.x).all() and torch.isfinite(batch.r).all()
    assert int(batch.a_index.min()) >= 0 and int(batch.a_index.max()) < net.num_actions
    roll.close(); env.close()


def _cli(ck, extra):
    return ["--agents", "24", "--arch", "weight_sharing", "--observed", "23", "--worlds", "64", "--episodes", "64", "--pretrain-steps", "0",
            "--print-every", "0", "--train-rows", "2048", "--checkpoint-dir", ck] + extra


def test_train_cli_on_the_ws_ring_kernels(tmp_path, capsys):
    from rl_collision_avoidance_amd.ga3c import train
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    ck = str(tmp_path / "ck")
    train.main(_cli(ck, ["--fused-crowd-ws"]))
    out = capsys.readouterr().out
    gb = FusedA3CTrainer.scratch_bytes(23, 2048, arch="weight_sharing") / 1e9
    assert ("policy: weight_sharing, 23 observed neighbours: the fused weight_sharing ring kernel for acting, the fused weight_sharing ring "
            "trainer kernels for training (%.1f GB of trainer scratch at --train-rows 2048)" % gb) in out
    assert "the autograd trainer" not in out
    assert "finished" in out
    files = sorted(glob.glob(ck + "/network_*.pt"))
    assert files
    state = torch.load(files[-1], map_location="cpu")
    assert state["arch"] == "weight_sharing" and state["max_others"] == 23 and state["training_step"] > 0
    assert "other_kernel" in state["model"]
    assert all(torch.isfinite(t).all() for t in state["model"].values() if torch.is_tensor(t) and t.is_floating_point())


@pytest.mark.parametrize("extra", [[], ["--fused-crowd-ws", "--autograd-trainer"]])
def test_train_cli_keeps_todays_line(extra, tmp_path, capsys):
    from rl_collision_avoidance_amd.ga3c import train
    train.main(_cli(str(tmp_path / "ck"), extra))
    out = capsys.readouterr().out
    assert TODAY in out
    assert "weight_sharing ring" not in out and "finished" in out


def test_train_cli_supervised_start_on_the_ws_ring_kernels(tmp_path, capsys):
    from rl_collision_avoidance_amd.ga3c import train
    args = _cli(str(tmp_path / "ck"), ["--fused-regression", "--fused-crowd-ws"])
    args[args.index("--pretrain-steps") + 1] = "3"
    train.main(args)
    out = capsys.readouterr().out
    assert "[Regression] on the fused weight_sharing trainer kernels" in out
    assert "[Regression] done" in out and "finished" in out
