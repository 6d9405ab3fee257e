"""CPU tests of the fused evaluation loop of crowd worlds with the weight_sharing network (`cavoid_crowd_eval_run_ws`,
csrc/cavoid_crowd_eval_ws.hpp; `ga3c.evaluate(fused_crowd_ws=True)`): the exported symbol and its argument check, the reasons the kernel
does not apply (host values only), what the three existing reason functions keep saying, the four switches of `evaluate`, the training
CLI's flag, the build's lists, and the built kernels' notes (profiles/crowd_ws_eval_resources.txt holds all the figures)."""
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
    decl = re.search(r"\bint\s+cavoid_crowd_eval_run_ws\s*\(([^;]*)\)\s*;", header)
    assert decl
    args = [a.strip() for a in re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", decl.group(1))).split(",")]
    assert len(args) == 13 and args[0] == "cavoid_env *env" and args[2] == "cavoid_policy *frozen" and args[3] == "const cavoid_eval_buffers *buffers"
    assert args[-1] == "void *stream"
    # the doc block in front of the declaration carries the definition of the return (the comment's line breaks folded)
    block = header[:decl.start()].rsplit("/*", 1)[1]
    folded = re.sub(r"\s*\n\s*\*\s*", " ", block)
    assert RETURN_SENTENCE in folded
    assert "CAVOID_FORM_CROWD_RVO" in folded and "worlds_running" in folded and "CAVOID_EUNSUPPORTED" in folded
    # the record struct is cavoid_eval_run's, declared once; the one-line form of the sentence stays where it was
    assert header.count("typedef struct cavoid_eval_buffers") == 1
    assert header.count(RETURN_SENTENCE) == 2


def test_library_exports_the_entry_point_and_checks_its_arguments():
    from rl_collision_avoidance_amd import _lib
    mine = [s for s in _lib.SYMBOLS if s[0] == "cavoid_crowd_eval_run_ws"]
    ws = [s for s in _lib.SYMBOLS if s[0] == "cavoid_eval_run_ws"]
    assert len(mine) == 1 and len(ws) == 1 and len(mine[0][2]) == 13
    assert mine[0][1] is ws[0][1] and mine[0][2] == ws[0][2]                      # cavoid_eval_run_ws's types
    fn = _lib.lib().cavoid_crowd_eval_run_ws                                      # (AttributeError if the library lacks it)
    assert fn(None, None, None, None, None, None, None, None, None, None, 2, 1, None) == -1         # CAVOID_EINVAL
    b = _lib.CavoidEvalBuffers()
    b.struct_size = C.sizeof(_lib.CavoidEvalBuffers)
    assert fn(None, None, None, C.byref(b), None, None, None, None, None, None, 0, 1, None) == -1    # ... before n_steps == 0 is looked at


# ---- the reasons that need no device (the stand-ins of tests/test_crowd_eval_host.py) ---------------------------------------------------
def _env(n, m=None, dynamics=0, frozen=0.0, nonlearning=0.0, rvo=0):
    m = n - 1 if m is None else m
    cfg = SimpleNamespace(dynamics=dynamics, gen_frozen_fraction=frozen, gen_nonlearning_fraction=nonlearning, rvo_enabled=rvo)
    return SimpleNamespace(max_agents=n, max_other=m, cfg=cfg)


def _fused(m, arch="weight_sharing", form=("split", 16), crowd=None, actions=11):
    ws = arch == "weight_sharing"
    return SimpleNamespace(act=lambda *a, **k: None, inference_form=("f32", 0) if ws else form, _h=object(), arch=arch, ws=ws,
                           crowd=(m > 19) if crowd is None else crowd, max_others=m, num_actions=actions)


def test_reason_is_none_for_what_the_kernel_carries():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate_fused_crowd_ws_unavailable_reason as why
    for n in range(17, 65):
        for m in (1, 7, 19, 20, n - 1):
            assert why(_env(n, m), _fused(m)) is None, (n, m)
    # both handle kinds: the whole-row handle (up to 19 neighbours) and the ring handle, which also serves a narrow row
    assert why(_env(20, 19), _fused(19, crowd=False)) is None and why(_env(20, 19), _fused(19, crowd=True)) is None
    assert why(_env(33, 7), _fused(7, crowd=True)) is None
    assert why(_env(20, 19, dynamics=1), _fused(19)) is None
    assert why(_env(20, 19, rvo=2, nonlearning=0.5), _fused(19)) is None          # scripted (ORCA) agents: the ORCA instantiation
    assert why(_env(40, 39, rvo=2, nonlearning=0.5), _fused(39)) is None
    assert why(_env(20, 19, frozen=0.3), _fused(19)) is None                      # (no scripted agents at all: none is frozen)
    # a matching frozen policy, of either kind, with or without agents for it
    assert why(_env(20, 19, frozen=0.3, nonlearning=0.5), _fused(19), _fused(19)) is None
    assert why(_env(40, 39, frozen=0.3, nonlearning=0.5, rvo=2), _fused(39), _fused(39)) is None
    assert why(_env(20, 19), _fused(19, crowd=False), _fused(19, crowd=True)) is None


def test_reason_names_each_refusal():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate_fused_crowd_ws_unavailable_reason as why
    unloaded = _fused(19)
    unloaded._h = None
    reasons = {
        "callable": why(_env(20, 19), lambda x: (x, x)),
        "rnn": why(_env(20, 19), _fused(19, arch="rnn")),
        "tile": why(_env(16, 15), _fused(15)),
        "holonomic": why(_env(20, 19, dynamics=2), _fused(19)),
        "neighbours": why(_env(20, 19), _fused(10)),
        "frozen policy": why(_env(20, 19), _fused(19), _fused(19, arch="rnn")),
        "frozen agents": why(_env(20, 19, frozen=0.3, nonlearning=0.5), _fused(19)),
    }
    assert all(isinstance(r, str) and r for r in reasons.values()), reasons
    assert len(set(reasons.values())) == len(reasons), reasons                    # a distinct string for each
    assert "FusedPolicy" in reasons["callable"]
    assert "rnn" in reasons["rnn"] and "fused_crowd=True" in reasons["rnn"] and "cavoid_crowd_eval_run" in reasons["rnn"]
    assert "16" in reasons["tile"] and "fused_ws=True" in reasons["tile"] and "cavoid_eval_run_ws" in reasons["tile"]
    for n in (1, 4):
        assert "cavoid_eval_run_ws" in why(_env(n, max(n - 1, 1)), _fused(max(n - 1, 1)))
    assert "holonomic" in reasons["holonomic"]
    assert "10" in reasons["neighbours"] and "19" in reasons["neighbours"] and "neighbours" in reasons["neighbours"]
    assert "frozen policy" in reasons["frozen policy"] and "rnn" in reasons["frozen policy"]
    # a frozen policy of another neighbour count, of another action count, or no FusedPolicy at all
    assert "frozen policy" in why(_env(20, 19), _fused(19), _fused(7))
    assert "frozen policy" in why(_env(20, 19), _fused(19), _fused(19, actions=5))
    assert "frozen policy" in why(_env(20, 19), _fused(19), unloaded)
    assert "frozen-network agents" in reasons["frozen agents"] and "frozen_policy" in reasons["frozen agents"]
    # the env step's LDS: cavoid_create admits no crowd env whose step exceeds what the pass lends it -- the widest there is fits
    from rl_collision_avoidance_amd.ga3c.rollout import WS_ACTOR_LENT_BYTES, crowd_env_step_lds_bytes
    assert max(crowd_env_step_lds_bytes(n, 6 + 7 * m) for n in range(17, 65) for m in (1, 19, n - 1)) <= min(65536, WS_ACTOR_LENT_BYTES)


def test_the_existing_reason_functions_say_what_they_said():
    from rl_collision_avoidance_amd.ga3c.evaluate import (evaluate_fused_crowd_unavailable_reason, evaluate_fused_unavailable_reason,
                                                          evaluate_fused_ws_unavailable_reason)
    rnn = lambda m: _fused(m, arch="rnn")
    assert evaluate_fused_unavailable_reason(_env(20, 19), rnn(19)) == "20 agents per world: crowd worlds (more than 16) are evaluated step by step"
    assert evaluate_fused_unavailable_reason(_env(64, 63), rnn(63)) == "64 agents per world: crowd worlds (more than 16) are evaluated step by step"
    ws = _fused(7)
    ws.crowd = False
    assert evaluate_fused_ws_unavailable_reason(_env(20, 7), ws) == "20 agents per world: crowd worlds (more than 16) are evaluated step by step"
    assert evaluate_fused_ws_unavailable_reason(_env(20, 19), rnn(19)) == (
        "the policy is the rnn network (use fused=True: cavoid_eval_run embeds the LSTM pass)")
    assert evaluate_fused_crowd_unavailable_reason(_env(20, 19), _fused(19)) == (
        "the policy is the weight_sharing network (the crowd evaluation kernel embeds the LSTM pass; the weight_sharing ring form is evaluated "
        "step by step)")
    assert evaluate_fused_crowd_unavailable_reason(_env(20, 19), rnn(19)) is None


def test_the_four_switches_exclude_each_other_and_raise_with_the_reason():
    import inspect
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate
    assert list(inspect.signature(evaluate).parameters)[-1] == "fused_crowd_ws"   # appended: positional callers keep their meaning
    assert inspect.signature(evaluate).parameters["fused_crowd_ws"].default is False
    names = ("fused", "fused_ws", "fused_crowd", "fused_crowd_ws")
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            with pytest.raises(ValueError, match="exclude"):
                evaluate(_env(20, 19), _fused(19), **{a: True, b: True})
    with pytest.raises(ValueError, match="exclude"):
        evaluate(_env(20, 19), _fused(19), fused=True, fused_ws=True, fused_crowd=True, fused_crowd_ws=True)
    # fused_crowd_ws=True raises with the reason, before anything touches a device
    with pytest.raises(ValueError, match=r"fused_crowd_ws=True.*FusedPolicy"):
        evaluate(_env(20, 19), lambda x: (x, x), fused_crowd_ws=True)
    with pytest.raises(ValueError, match=r"fused_crowd_ws=True.*cavoid_eval_run_ws"):
        evaluate(_env(4, 3), _fused(3), fused_crowd_ws=True)
    with pytest.raises(ValueError, match=r"fused_crowd_ws=True.*cavoid_crowd_eval_run"):
        evaluate(_env(20, 19), _fused(19, arch="rnn"), fused_crowd_ws=True)
    with pytest.raises(ValueError, match="frozen policy"):
        evaluate(_env(20, 19), _fused(19), fused_crowd_ws=True, frozen_policy=_fused(19, arch="rnn"))
    with pytest.raises(ValueError, match="steps_per_launch"):
        evaluate(_env(20, 19), _fused(19), fused_crowd_ws=True, steps_per_launch=0)
    # the others still raise in their old words on these inputs
    with pytest.raises(ValueError, match="crowd worlds \\(more than 16\\) are evaluated step by step"):
        evaluate(_env(20, 7), _fused(7, crowd=False), fused_ws=True)
    with pytest.raises(ValueError, match="the weight_sharing ring form is evaluated step by step"):
        evaluate(_env(20, 19), _fused(19), fused_crowd=True)


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
    base = ["--agents", "20", "--arch", "weight_sharing", "--evaluate", "1"]
    for argv, want in ((base + ["--fused-crowd-ws-evaluate"], True), (base, False)):
        with pytest.raises(Stop):
            train.main(argv)
        assert seen["args"].fused_crowd_ws_evaluate is want
        assert seen["args"].fused_evaluate is False and seen["args"].fused_ws_evaluate is False and seen["args"].fused_crowd_evaluate is False
    monkeypatch.undo()
    src = open(os.path.join(ROOT, "rl_collision_avoidance_amd", "ga3c", "train.py")).read()
    assert '"[Evaluate] fused crowd weight_sharing evaluation kernel (cavoid_crowd_eval_run_ws), %d env steps per launch"' in src
    assert "--fused-crowd-ws-evaluate: the fused crowd weight_sharing evaluation kernel (cavoid_crowd_eval_run_ws) does not" in src


def test_build_lists_the_unit_with_the_licm_flag():
    from rl_collision_avoidance_amd import build
    name = "cavoid_crowd_eval_ws.hip"
    assert [os.path.basename(s) for s in build.SOURCES].count(name) == 1
    assert build.EXTRA_FLAGS[name] == ["-mllvm", "-disable-machine-licm"]
    heads = build.HEADERS[name]
    for h in ("cavoid_crowd_eval_ws.hpp", "cavoid_crowd_actor_ws.hpp", "cavoid_eval_ws.hpp", "cavoid_crowd_actor.hpp", "cavoid_actor_ws.hpp",
              "cavoid_crowd.hpp", "cavoid_crowd_rvo.hpp", "cavoid_eval.hpp", "cavoid_eval_host.hpp", "cavoid_policy_ws.hpp", "cavoid_policy_wsring.hpp",
              "cavoid_policy_pipe.hpp", "cavoid_kernels.hpp", "cavoid_launch.hpp"):
        assert h in heads, h
    assert all(os.path.exists(os.path.join(build.CSRC, h)) for h in heads)
    assert os.path.join(build.CSRC, "cavoid_crowd_eval_ws.hpp") in build.DEPS     # (the source digest covers it)
    # every header the unit's own header chain includes by name is listed
    seen, todo = set(), ["cavoid_crowd_eval_ws.hip"]
    while todo:
        f = todo.pop()
        for inc in re.findall(r'#include\s+"(cavoid_\w+\.hpp)"', open(os.path.join(build.CSRC, f)).read()):
            if inc not in seen:
                seen.add(inc); todo.append(inc)
    assert seen <= set(heads), sorted(seen - set(heads))


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))),
                    reason="llvm-objdump / llvm-readelf of the ROCm toolchain not present")
def test_crowd_ws_evaluation_kernels_fit_two_workgroups_per_cu_without_scratch():
    """no scratch and at most 256 registers are CONDITIONS of two workgroups of four wavefronts per CU (512 registers per SIMD lane), not
    measurements"""
    text = _kernel_notes()
    found = re.findall(r"\.name:\s+(\S*crowd_ws_evaluate_kernel\S*)\s*\n\s*\.private_segment_fixed_size:\s+(\d+)", text)
    # two buckets of the agent count (32, 64) x (plain, ORCA-carrying env step) x (one network, a second frozen one)
    assert len(found) == 8, found
    want = sorted((nb, r, f) for nb in ("32", "64") for r in "01" for f in "01")
    assert sorted(re.search(r"crowd_ws_evaluate_kernelILi(\d+)ELb(\d)ELb(\d)E", name).groups() for name, _ in found) == want
    assert all(int(size) == 0 for _, size in found), found
    # one workgroup of four wavefronts per crowd tile
    sizes = re.findall(r"\.max_flat_workgroup_size:\s+(\d+)\s*\n\s*\.name:\s+\S*crowd_ws_evaluate_kernel", text)
    assert sizes == ["256"] * 8, sizes
    vgprs = re.findall(r"\.name:\s+\S*crowd_ws_evaluate_kernel\S*\s*\n(?:\s+\.(?!name)\S+:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text)
    assert len(vgprs) == 8 and all(int(v) <= 256 for v in vgprs), vgprs
    # the names stay clear of the substrings other tests count kernels by
    clash = r"eval_kernel|eval_ws_kernel|actor_kernel|actor_ws_kernel|crowd_kernel|crowd_evaluate_kernel|crowd_ws_rollout_kernel"
    assert not any(re.search(clash, name) for name, _ in found), found
