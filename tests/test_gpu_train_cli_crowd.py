"""ga3c.train on crowd worlds with --fused-crowd-trainer: 64-agent worlds act on the fused crowd policy kernel, drain rows of 446 floats and
train on the ring trainer kernels; without the flag every line stays what tests/test_gpu_policy_crowd.py pins."""
import glob

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


def _cli(agents, ck, extra):
    return ["--agents", str(agents), "--worlds", "64", "--episodes", "64", "--pretrain-steps", "0", "--print-every", "0", "--train-rows", "2048",
            "--checkpoint-dir", ck] + extra


def test_train_cli_on_the_ring_trainer(tmp_path, capsys):
    from rl_collision_avoidance_amd.ga3c import train
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    ck = str(tmp_path / "ck")
    train.main(_cli(64, ck, ["--fused-crowd-trainer"]))
    out = capsys.readouterr().out
    gb = FusedA3CTrainer.scratch_bytes(63, 2048) / 1e9
    assert ("policy: the fused crowd policy kernel for acting, the fused ring trainer kernels for training (63 observed neighbours, "
            "%.1f GB of trainer scratch at --train-rows 2048)" % gb) in out
    assert "the autograd trainer" not in out
    assert "finished" in out
    files = sorted(glob.glob(ck + "/network_*.pt"))
    assert files
    state = torch.load(files[-1], map_location="cpu")
    assert state["training_step"] > 0 and "lstm_kernel" in state["model"]
    assert all(torch.isfinite(t).all() for t in state["model"].values() if torch.is_tensor(t) and t.is_floating_point())


def test_train_cli_without_the_flag_keeps_the_autograd_line(tmp_path, capsys):
    from rl_collision_avoidance_amd.ga3c import train
    train.main(_cli(32, str(tmp_path / "ck"), []))
    out = capsys.readouterr().out
    assert "policy: the fused crowd policy kernel for acting, the autograd trainer" in out
    assert "ring trainer" not in out and "finished" in out


@pytest.mark.parametrize("extra", [["--autograd-trainer"], ["--torch-policy"]])
def test_the_flag_yields_to_the_pytorch_switches(extra, tmp_path, capsys):
    from rl_collision_avoidance_amd.ga3c import train
    train.main(_cli(24, str(tmp_path / "ck"), ["--fused-crowd-trainer"] + extra))
    out = capsys.readouterr().out
    assert "the autograd trainer" in out and "ring trainer" not in out and "finished" in out
