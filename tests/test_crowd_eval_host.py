"""CPU tests of the fused evaluation loop of crowd worlds (`cavoid_crowd_eval_run`, csrc/cavoid_crowd_eval.hpp;
`ga3c.evaluate(fused_crowd=True)`): the exported symbol and its argument check, the reasons the kernel does not apply (host values only),
what the two existing reason functions keep saying, the training CLI's flag, the build's lists, and the built kernels' scratch
(profiles/crowd_eval_resources.txt holds all the figures)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

from tests.host_support import LLVM, ROOT, _kernel_notes

RETURN_SENTENCE = "An agent's return sums the rewards up to and including the step at which its world is over."


def test_header_declares_the_entry_point_with_the_return_sentence():
    header = open(os.path.join(ROOT, "include", "cavoid.h")).read()
    assert re.search(r"#define\s+CAVOID_ABI_VERSION\s+3\b", header)              # additive: the version stays
    decl = re.search(r"\bint\s+cavoid_crowd_eval_run\s*\(([^;]*)\)\s*;", header)
    assert decl
    args = [a.strip() for a in re.sub(r"\s+", " ", decl.group(1)).split(",")]
    assert len(args) == 12 and args[0] == "cavoid_env *env" and args[2] == "const cavoid_eval_buffers *buffers" and args[-1] == "void *stream"
    # the doc block in front of the declaration carries the definition of the return (the comment's line breaks folded)
    block = header[:decl.start()].rsplit("/*", 1)[1]
    folded = re.sub(r"\s*\n\s*\*\s*", " ", block)
    assert RETURN_SENTENCE in folded
    assert "CAVOID_FORM_CROWD_RVO" in folded and "worlds_running" in folded and "CAVOID_EUNSUPPORTED" in folded
    # the record struct is cavoid_eval_run's, declared once
    assert header.count("typedef struct cavoid_eval_buffers") == 1


def test_library_exports_the_entry_point_and_checks_its_arguments():
    from rl_collision_avoidance_amd import _lib
    mine = [s for s in _lib.SYMBOLS if s[0] == "cavoid_crowd_eval_run"]
    plain = [s for s in _lib.SYMBOLS if s[0] == "cavoid_eval_run"]
    assert len(mine) == 1 and len(mine[0][2]) == 12
    # cavoid_eval_run's argument list without the frozen handle
    assert mine[0][1] is plain[0][1] and mine[0][2] == plain[0][2][:2] + plain[0][2][3:]
    fn = _lib.lib().cavoid_crowd_eval_run                                         # (AttributeError if the library lacks it)
    assert fn(None, None, None, None, None, None, None, None, None, 2, 1, None) == -1        # CAVOID_EINVAL
    b = _lib.CavoidEvalBuffers()
    b.struct_size = C.sizeof(_lib.CavoidEvalBuffers)
    assert fn(None, None, C.byref(b), None, None, None, None, None, None, 0, 1, None) == -1   # ... before n_steps == 0 is looked at


# ---- the reasons that need no device ------------------------------------------------------------------------------------------------
def _env(n, m=None, dynamics=0, frozen=0.0, nonlearning=0.0, rvo=0):
    m = n - 1 if m is None else m
    cfg = SimpleNamespace(dynamics=dynamics, gen_frozen_fraction=frozen, gen_nonlearning_fraction=nonlearning, rvo_enabled=rvo)
    return SimpleNamespace(max_agents=n, max_other=m, cfg=cfg)


def _fused(m, arch="rnn", form=("split", 16)):
    ws = arch == "weight_sharing"
    return SimpleNamespace(act=lambda *a, **k: None, inference_form=("f32", 0) if ws else form, _h=object(), arch=arch, ws=ws,
                           crowd=m > 19, max_others=m, num_actions=11)


def test_reason_is_none_for_what_the_kernel_carries():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate_fused_crowd_unavailable_reason as why
    for n in range(17, 65):
        for m in (1, 16, 19, 20, n - 1):
            assert why(_env(n, m), _fused(m)) is None, (n, m)
    assert why(_env(20, 19, dynamics=1), _fused(19)) is None
    assert why(_env(20, 19, rvo=2, nonlearning=0.5), _fused(19)) is None          # scripted (ORCA) agents: the ORCA instantiation
    assert why(_env(20, 19, frozen=0.3), _fused(19)) is None                      # (no scripted agents at all: none is frozen)


def test_reason_names_each_refusal():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate_fused_crowd_unavailable_reason as why
    reasons = {
        "tile": why(_env(16, 15), _fused(15)),
        "ws": why(_env(20, 19), _fused(19, arch="weight_sharing")),
        "holonomic": why(_env(20, 19, dynamics=2), _fused(19)),
        "frozen agents": why(_env(20, 19, frozen=0.3, nonlearning=0.5), _fused(19)),
        "frozen policy": why(_env(20, 19), _fused(19), _fused(19)),
        "form": why(_env(33, 32), _fused(32, form=("split", 3))),
        "neighbours": why(_env(20, 19), _fused(10)),
        "callable": why(_env(20, 19), lambda x: (x, x)),
    }
    assert all(isinstance(r, str) and r for r in reasons.values()), reasons
    assert len(set(reasons.values())) == len(reasons), reasons                    # a distinct string for each
    assert "16" in reasons["tile"] and "cavoid_eval_run" in reasons["tile"]
    for n in (1, 4):
        assert "cavoid_eval_run" in why(_env(n, max(n - 1, 1)), _fused(max(n - 1, 1)))
    assert "weight_sharing" in reasons["ws"]
    assert "holonomic" in reasons["holonomic"]
    assert "frozen-network agents" in reasons["frozen agents"]
    assert "frozen_policy" in reasons["frozen policy"]
    assert "non-default inference form" in reasons["form"] and "non-default inference form" in why(_env(33, 32), _fused(32, form=("f32", 0)))
    assert "10" in reasons["neighbours"] and "19" in reasons["neighbours"] and "neighbours" in reasons["neighbours"]
    assert "FusedPolicy" in reasons["callable"]


def test_the_existing_reason_functions_say_what_they_said():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate_fused_unavailable_reason, evaluate_fused_ws_unavailable_reason
    assert evaluate_fused_unavailable_reason(_env(20, 19), _fused(19)) == "20 agents per world: crowd worlds (more than 16) are evaluated step by step"
    assert evaluate_fused_unavailable_reason(_env(64, 63), _fused(63)) == "64 agents per world: crowd worlds (more than 16) are evaluated step by step"
    ws = _fused(7, arch="weight_sharing")
    ws.crowd = False
    assert evaluate_fused_ws_unavailable_reason(_env(20, 7), ws) == "20 agents per world: crowd worlds (more than 16) are evaluated step by step"
    assert evaluate_fused_ws_unavailable_reason(_env(20, 19), _fused(19)) == (
        "the policy is the rnn network (use fused=True: cavoid_eval_run embeds the LSTM pass)")


def test_the_switches_exclude_each_other_and_raise_with_the_reason():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate
    for other in (dict(fused=True), dict(fused_ws=True), dict(fused=True, fused_ws=True)):
        with pytest.raises(ValueError, match="exclude"):
            evaluate(_env(20, 19), _fused(19), fused_crowd=True, **other)
    # fused_crowd=True raises with the reason, before anything touches a device
    with pytest.raises(ValueError, match=r"fused_crowd=True.*FusedPolicy"):
        evaluate(_env(20, 19), lambda x: (x, x), fused_crowd=True)
    with pytest.raises(ValueError, match=r"fused_crowd=True.*cavoid_eval_run"):
        evaluate(_env(4, 3), _fused(3), fused_crowd=True)
    with pytest.raises(ValueError, match="frozen_policy"):
        evaluate(_env(20, 19), _fused(19), fused_crowd=True, frozen_policy=_fused(19))
    with pytest.raises(ValueError, match="steps_per_launch"):
        evaluate(_env(20, 19), _fused(19), fused_crowd=True, steps_per_launch=0)


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
    for argv, want in ((["--agents", "20", "--evaluate", "1", "--fused-crowd-evaluate"], True), (["--agents", "20", "--evaluate", "1"], False)):
        with pytest.raises(Stop):
            train.main(argv)
        assert seen["args"].fused_crowd_evaluate is want
        assert seen["args"].fused_evaluate is False and seen["args"].fused_ws_evaluate is False
    monkeypatch.undo()
    src = open(os.path.join(ROOT, "rl_collision_avoidance_amd", "ga3c", "train.py")).read()
    assert '"[Evaluate] fused crowd evaluation kernel (cavoid_crowd_eval_run), %d env steps per launch"' in src


def test_build_lists_the_unit_with_the_licm_flag():
    from rl_collision_avoidance_amd import build
    name = "cavoid_crowd_eval.hip"
    assert [os.path.basename(s) for s in build.SOURCES].count(name) == 1
    assert build.EXTRA_FLAGS[name] == ["-mllvm", "-disable-machine-licm"]
    heads = build.HEADERS[name]
    for h in ("cavoid_crowd_eval.hpp", "cavoid_crowd_actor.hpp", "cavoid_crowd.hpp", "cavoid_crowd_rvo.hpp", "cavoid_eval.hpp", "cavoid_eval_host.hpp",
              "cavoid_policy_crowd.hpp", "cavoid_policy_split.hpp", "cavoid_kernels.hpp", "cavoid_launch.hpp"):
        assert h in heads, h
    assert all(os.path.exists(os.path.join(build.CSRC, h)) for h in heads)
    assert os.path.join(build.CSRC, "cavoid_crowd_eval.hpp") in build.DEPS        # (the source digest covers it)


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))),
                    reason="llvm-objdump / llvm-readelf of the ROCm toolchain not present")
def test_crowd_evaluation_kernels_use_no_scratch():
    text = _kernel_notes()
    found = re.findall(r"\.name:\s+(\S*crowd_evaluate_kernel\S*)\s*\n\s*\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(found) == 4, found            # two buckets of the agent count (32, 64) x (plain, ORCA-carrying env step)
    assert all(int(size) == 0 for _, size in found), found
    assert sorted(re.search(r"crowd_evaluate_kernelILi(\d+)ELb(\d)E", name).groups() for name, _ in found) == [("32", "0"), ("32", "1"), ("64", "0"), ("64", "1")]
    # one workgroup of four wavefronts per crowd tile
    sizes = re.findall(r"\.max_flat_workgroup_size:\s+(\d+)\s*\n\s*\.name:\s+\S*crowd_evaluate_kernel", text)
    assert sizes == ["256"] * 4, sizes
    # the names stay clear of the substrings other tests count kernels by
    assert not any(re.search(r"eval_kernel|eval_ws_kernel|actor_kernel|crowd_kernel|crowd_push_kernel|crowd_rvo_kernel", name) for name, _ in found)
