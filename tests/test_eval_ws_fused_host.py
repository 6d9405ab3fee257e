"""CPU tests of the fused evaluation loop of the weight-sharing network (`cavoid_eval_run_ws`, csrc/cavoid_eval_ws.hpp;
`ga3c.evaluate(fused_ws=True)`): the exported symbol and its argument check, the training CLI's flag, the reasons the kernel does not
apply that need no device, and the built kernels' registers and scratch (profiles/eval_ws_resources.txt holds all of them)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

from tests.host_support import LLVM, ROOT, _kernel_notes


def test_library_exports_the_entry_point_and_checks_its_arguments():
    from rl_collision_avoidance_amd import _lib
    header = open(os.path.join(ROOT, "include", "cavoid.h")).read()
    assert re.search(r"\bint\s+cavoid_eval_run_ws\s*\(", header)
    assert re.search(r"#define\s+CAVOID_ABI_VERSION\s+3\b", header)              # additive: the version stays
    # the same definition of the return as cavoid_eval_run's, in both doc blocks
    assert header.count("An agent's return sums the rewards up to and including the step at which its world is over.") == 2
    ws = [(name, res, args) for name, res, args in _lib.SYMBOLS if name == "cavoid_eval_run_ws"]
    plain = [(name, res, args) for name, res, args in _lib.SYMBOLS if name == "cavoid_eval_run"]
    assert len(ws) == 1 and len(plain) == 1 and ws[0][1:] == plain[0][1:]        # cavoid_eval_run's signature
    fn = _lib.lib().cavoid_eval_run_ws                                            # (AttributeError if the library lacks it)
    assert fn(None, None, None, None, None, None, None, None, None, None, 2, 1, None) == -1       # CAVOID_EINVAL
    b = _lib.CavoidEvalBuffers()
    b.struct_size = C.sizeof(_lib.CavoidEvalBuffers)
    assert fn(None, None, None, C.byref(b), None, None, None, None, None, None, 0, 1, None) == -1  # ... before n_steps == 0 is looked at


def test_train_cli_knows_the_flag(monkeypatch):
    import argparse
    from rl_collision_avoidance_amd.ga3c import train
    seen = {}

    class Stop(Exception):
        pass

    def parse(self, argv=None):
        seen["args"] = argparse.ArgumentParser.parse_known_args(self, argv)[0]
        raise Stop()
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    for argv, want in ((["--evaluate", "1", "--arch", "weight_sharing", "--fused-ws-evaluate"], True), (["--evaluate", "1"], False)):
        with pytest.raises(Stop):
            train.main(argv)
        assert seen["args"].fused_ws_evaluate is want and seen["args"].fused_evaluate is False
    monkeypatch.undo()
    src = open(os.path.join(ROOT, "rl_collision_avoidance_amd", "ga3c", "train.py")).read()
    assert '"[Evaluate] fused weight_sharing evaluation kernel (cavoid_eval_run_ws), %d env steps per launch"' in src


# ---- the reasons that need no device ------------------------------------------------------------------------------------------------
def _env(n, m=None, dynamics=0, frozen=0.0, nonlearning=0.0, rvo=0):
    m = n - 1 if m is None else m
    cfg = SimpleNamespace(dynamics=dynamics, gen_frozen_fraction=frozen, gen_nonlearning_fraction=nonlearning, rvo_enabled=rvo)
    return SimpleNamespace(max_agents=n, max_other=m, cfg=cfg)


def _fused(m, arch="weight_sharing", ring=False, actions=11):
    ws = arch == "weight_sharing"
    return SimpleNamespace(act=lambda *a, **k: None, inference_form=("f32", 0) if ws else ("split", 16), _h=object(), arch=arch, ws=ws,
                           crowd=ring or m > 19, max_others=m, num_actions=actions)


def test_reasons_without_a_device():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate, evaluate_fused_unavailable_reason, evaluate_fused_ws_unavailable_reason as why
    for n in (1, 2, 4, 10, 16):
        assert why(_env(n, max(n - 1, 1)), _fused(max(n - 1, 1))) is None
    assert why(_env(4, 7), _fused(7)) is None                                     # WS-8: slots past the neighbour count
    assert why(_env(16, 19), _fused(19)) is None                                  # the widest parked row
    assert why(_env(4, 7, rvo=1, nonlearning=0.5), _fused(7)) is None
    assert why(_env(4, 7, frozen=0.3, nonlearning=0.5), _fused(7), _fused(7)) is None
    # one per refusal of the C entry point ...
    r = why(_env(4, 3), _fused(3, arch="rnn"))
    assert "rnn" in r and "fused=True" in r
    r = why(_env(4, 24), _fused(24, ring=True))
    assert "ring" in r and "24" in r and "19" in r
    r = why(_env(20, 19), _fused(19))
    assert "crowd" in r and "20" in r and "16" in r
    assert "holonomic" in why(_env(4, 7, dynamics=2), _fused(7))
    r = why(_env(4, 7, frozen=0.3, nonlearning=0.5), _fused(7), _fused(7, arch="rnn"))
    assert "frozen policy" in r and "rnn" in r
    assert "frozen policy" in why(_env(4, 7, frozen=0.3, nonlearning=0.5), _fused(7), _fused(5))
    assert "frozen policy" in why(_env(4, 7, frozen=0.3, nonlearning=0.5), _fused(7), _fused(7, actions=7))
    r = why(_env(4, 7, frozen=0.3, nonlearning=0.5), _fused(7))
    assert "frozen-network agents without a frozen_policy" in r
    r = why(_env(16, 15, rvo=1), _fused(15))
    assert "LDS" in r and "66560" in r
    # ... and the three that are Python's alone
    assert "FusedPolicy" in why(_env(4, 7), lambda x: (x, x))
    r = why(_env(4, 3), _fused(7))
    assert "7" in r and "3" in r and "neighbours" in r
    # evaluate(fused=True) keeps naming the network for a weight_sharing policy
    assert "weight_sharing" in evaluate_fused_unavailable_reason(_env(4, 7), _fused(7))
    # fused_ws=True raises with the reason, before anything touches a device; both flags together are refused
    with pytest.raises(ValueError, match="FusedPolicy"):
        evaluate(_env(4, 7), lambda x: (x, x), fused_ws=True)
    with pytest.raises(ValueError, match="fused_ws=True.*rnn"):
        evaluate(_env(4, 3), _fused(3, arch="rnn"), fused_ws=True)
    with pytest.raises(ValueError, match="exclude each other"):
        evaluate(_env(4, 7), _fused(7), fused=True, fused_ws=True)


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))),
                    reason="llvm-objdump / llvm-readelf of the ROCm toolchain not present")
def test_eval_ws_kernels_take_no_scratch_and_no_more_registers_than_the_actor():
    text = _kernel_notes()
    pat = r"\.name:\s+\S*%sILi(\d+)ELb(\d)ELb(\d)E\S*\s*\n\s*\.private_segment_fixed_size:\s+(\d+)"
    found = {k[:3]: int(k[3]) for k in re.findall(pat % "eval_ws_kernel", text)}
    assert len(found) == 48, sorted(found)                   # 1..16 agents x (plain, ORCA, ORCA + frozen network)
    assert sorted(found) == sorted((str(n), r, f) for n in range(1, 17) for r, f in (("0", "0"), ("1", "0"), ("1", "1")))
    assert found[("4", "0", "0")] == 0 and found[("10", "0", "0")] == 0
    vg = r"\.name:\s+\S*%s\S*\s*\n(?:\s+\.(?!name)\S+:.*\n)*?\s+\.vgpr_count:\s+(\d+)"
    ev = {k[:3]: int(k[3]) for k in re.findall(vg % r"eval_ws_kernelILi(\d+)ELb(\d)ELb(\d)E", text)}
    ac = {k[:2]: int(k[2]) for k in re.findall(vg % r"actor_ws_kernelILi(\d+)ELb(\d)E", text)}
    assert len(ev) == 48 and len(ac) == 32
    for n in ("4", "10"):
        assert ev[(n, "0", "0")] <= ac[(n, "0")], (n, ev[(n, "0", "0")], ac[(n, "0")])
    assert all(v <= 256 for v in ev.values()), ev
    sizes = re.findall(r"\.max_flat_workgroup_size:\s+(\d+)\s*\n\s*\.name:\s+\S*eval_ws_kernel", text)
    assert sizes == ["256"] * 48, sizes
    # the kernel's name keeps clear of the two the other host tests count by
    assert "eval_kernel" not in "eval_ws_kernel" and "actor_ws_kernel" not in "eval_ws_kernel"
