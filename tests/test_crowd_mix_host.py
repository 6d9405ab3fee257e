"""CPU tests of the crowd launches that carry frozen-network agents (`cavoid_crowd_actor_run_mix`, csrc/cavoid_crowd_actor_mix.hpp;
`cavoid_crowd_eval_run_mix`, csrc/cavoid_crowd_eval_mix.hpp; `BatchedRollout.run_fused_crowd_mix`, `ga3c.evaluate(fused_crowd_mix=True)`):
the declarations and exported symbols with their argument checks, the two new reason functions (host values only), what the existing
reason functions and switches keep saying for frozen cases, the five switches of `evaluate`, the training CLI's flags, the build's lists,
and the built kernels' notes (profiles/crowd_mix_resources.txt holds all the figures)."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

from tests.host_support import LLVM, ROOT, _kernel_notes

RETURN_SENTENCE = "An agent's return sums the rewards up to and including the step at which its world is over."


def _decl(header, name):
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert decl, name
    args = [a.strip() for a in re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", decl.group(1))).split(",")]
    block = header[:decl.start()].rsplit("/*", 1)[1]
    return args, re.sub(r"\s*\n\s*\*\s*", " ", block)


def test_header_declares_both_entry_points():
    header = open(os.path.join(ROOT, "include", "cavoid.h")).read()
    assert re.search(r"#define\s+CAVOID_ABI_VERSION\s+3\b", header)              # additive: the version stays
    args, doc = _decl(header, "cavoid_crowd_actor_run_mix")
    mix_args, _ = _decl(header, "cavoid_actor_run_mix")
    assert len(args) == 15 and args == mix_args                                  # cavoid_actor_run_mix's argument list
    assert args[2] == "cavoid_policy *frozen" and args[3] == "cavoid_rollout *rollout" and args[-1] == "void *stream"
    assert "CAVOID_EUNSUPPORTED" in doc and "CAVOID_EINVAL" in doc and "n_steps == 0" in doc and "CAVOID_POLICY_FROZEN_NET" in doc
    args, doc = _decl(header, "cavoid_crowd_eval_run_mix")
    eval_args, _ = _decl(header, "cavoid_eval_run")
    assert len(args) == 13 and args == eval_args                                 # cavoid_eval_run's argument list; `frozen` is required here
    assert args[2] == "cavoid_policy *frozen" and args[3] == "const cavoid_eval_buffers *buffers"
    assert RETURN_SENTENCE in doc                                                # the definition of the return, with the comment's line breaks folded
    assert "worlds_running" in doc and "CAVOID_EUNSUPPORTED" in doc and "REQUIRED" in doc
    assert header.count(RETURN_SENTENCE) == 2                                    # the one-line form of the sentence stays where it was
    # the refusal notes of the one-network launches point to the new ones
    assert "cavoid_crowd_actor_run_mix" in _decl(header, "cavoid_crowd_actor_run")[1]
    assert "cavoid_crowd_eval_run_mix" in _decl(header, "cavoid_crowd_eval_run")[1]


def test_library_exports_both_entry_points_and_checks_their_arguments():
    from rl_collision_avoidance_amd import _lib
    sym = {s[0]: s for s in _lib.SYMBOLS}
    assert sym["cavoid_crowd_actor_run_mix"][1:] == sym["cavoid_actor_run_mix"][1:] and len(sym["cavoid_crowd_actor_run_mix"][2]) == 15
    assert sym["cavoid_crowd_eval_run_mix"][1:] == sym["cavoid_eval_run"][1:] and len(sym["cavoid_crowd_eval_run_mix"][2]) == 13
    actor = _lib.lib().cavoid_crowd_actor_run_mix                                 # (AttributeError if the library lacks it)
    evalf = _lib.lib().cavoid_crowd_eval_run_mix
    assert actor(*([None] * 12), 2, 1, None) == -1                                # CAVOID_EINVAL
    rb = _lib.CavoidRolloutBuffers()
    rb.struct_size = C.sizeof(_lib.CavoidRolloutBuffers)
    assert actor(None, None, None, None, C.byref(rb), *([None] * 7), 0, 1, None) == -1     # ... before n_steps == 0 is looked at
    assert evalf(*([None] * 10), 2, 1, None) == -1
    eb = _lib.CavoidEvalBuffers()
    eb.struct_size = C.sizeof(_lib.CavoidEvalBuffers)
    assert evalf(None, None, None, C.byref(eb), *([None] * 6), 0, 1, None) == -1


# ---- the reasons that need no device --------------------------------------------------------------------------------------------------
def _env(n, m=None, dynamics=0, frozen=0.5, nonlearning=0.5, rvo=0):
    m = n - 1 if m is None else m
    cfg = SimpleNamespace(dynamics=dynamics, gen_frozen_fraction=frozen, gen_nonlearning_fraction=nonlearning, rvo_enabled=rvo, max_other=m)
    return SimpleNamespace(max_agents=n, max_other=m, cfg=cfg)


def _fused(m, arch="rnn", form=("split", 16), actions=11):
    ws = arch == "weight_sharing"
    return SimpleNamespace(act=lambda *a, **k: None, inference_form=("f32", 0) if ws else form, _h=object(), arch=arch, ws=ws, crowd=ws and m > 19,
                           max_others=m, num_actions=actions, accepts_strided_obs=True)


def test_both_reasons_are_none_for_what_the_kernels_carry():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate_fused_crowd_mix_unavailable_reason as why_eval
    from rl_collision_avoidance_amd.ga3c.rollout import crowd_actor_mix_unavailable_reason as why_actor
    for n in range(17, 65):
        for m in (1, 16, 19, 20, n - 1):
            assert why_eval(_env(n, m), _fused(m), _fused(m)) is None, (n, m)
            assert why_actor(n, 0, "rnn", ("split", 16), m, m, "rnn", ("split", 16), m) is None, (n, m)
    assert why_eval(_env(20, 19, dynamics=1), _fused(19), _fused(19)) is None
    assert why_eval(_env(40, 39, rvo=2), _fused(39), _fused(39)) is None
    assert why_eval(_env(20, 19, frozen=0.0), _fused(19), _fused(19)) is None     # no frozen-network agents: the second pass never runs
    assert why_actor(40, 1, "rnn", ("split", 16), 39, 39, "rnn", ("split", 16), 39) is None


def test_both_reasons_name_each_refusal():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate_fused_crowd_mix_unavailable_reason as why_eval
    from rl_collision_avoidance_amd.ga3c.rollout import crowd_actor_mix_unavailable_reason as why_actor
    unloaded = _fused(19)
    unloaded._h = None
    ev = {
        "callable": why_eval(_env(20, 19), lambda x: (x, x), _fused(19)),
        "tile": why_eval(_env(16, 15), _fused(15), _fused(15)),
        "ws": why_eval(_env(20, 19), _fused(19, arch="weight_sharing"), _fused(19)),
        "holonomic": why_eval(_env(20, 19, dynamics=2), _fused(19), _fused(19)),
        "form": why_eval(_env(20, 19), _fused(19, form=("split", 3)), _fused(19)),
        "neighbours": why_eval(_env(20, 19), _fused(10), _fused(10)),
        "no frozen": why_eval(_env(20, 19), _fused(19), None),
        "frozen unloaded": why_eval(_env(20, 19), _fused(19), unloaded),
        "frozen ws": why_eval(_env(20, 19), _fused(19), _fused(19, arch="weight_sharing")),
        "frozen form": why_eval(_env(20, 19), _fused(19), _fused(19, form=("f32", 0))),
        "frozen narrower": why_eval(_env(20, 19), _fused(19), _fused(10)),
        "frozen actions": why_eval(_env(20, 19), _fused(19), _fused(19, actions=5)),
    }
    ac = {
        "tile": why_actor(16, 0, "rnn", ("split", 16), 15, 15, "rnn", ("split", 16), 15),
        "no FusedPolicy": why_actor(20, 0, "rnn", ("split", 16), 19, 19, "rnn", ("split", 16), 19, fused_policy=False),
        "ws": why_actor(20, 0, "weight_sharing", ("f32", 0), 19, 19, "rnn", ("split", 16), 19),
        "holonomic": why_actor(20, 2, "rnn", ("split", 16), 19, 19, "rnn", ("split", 16), 19),
        "form": why_actor(20, 0, "rnn", ("split", 3), 19, 19, "rnn", ("split", 16), 19),
        "neighbours": why_actor(20, 0, "rnn", ("split", 16), 10, 19, "rnn", ("split", 16), 10),
        "no frozen": why_actor(20, 0, "rnn", ("split", 16), 19, 19, None),
        "frozen no FusedPolicy": why_actor(20, 0, "rnn", ("split", 16), 19, 19, "rnn", ("split", 16), 19, frozen_fused_policy=False),
        "frozen ws": why_actor(20, 0, "rnn", ("split", 16), 19, 19, "weight_sharing", ("f32", 0), 19),
        "frozen form": why_actor(20, 0, "rnn", ("split", 16), 19, 19, "rnn", ("split", 3), 19),
        "frozen narrower": why_actor(20, 0, "rnn", ("split", 16), 19, 19, "rnn", ("split", 16), 10),
    }
    for reasons in (ev, ac):
        assert all(isinstance(r, str) and r for r in reasons.values()), reasons
        assert len(set(reasons.values())) == len(reasons), reasons                # a distinct string for each
        assert "holonomic" in reasons["holonomic"] and "weight_sharing" in reasons["ws"]
        assert "10" in reasons["neighbours"] and "19" in reasons["neighbours"]
        assert "frozen policy" in reasons["frozen ws"] and "weight_sharing" in reasons["frozen ws"]
        assert "frozen policy" in reasons["frozen narrower"] and "10" in reasons["frozen narrower"]
        assert "frozen policy" in reasons["frozen form"]
    assert "cavoid_eval_run" in ev["tile"] and "fused=True" in ev["tile"]
    assert "cavoid_actor_run_mix" in ac["tile"] and "run_fused" in ac["tile"]
    # without a frozen policy the reason points to the one-network form
    assert "fused_crowd=True" in ev["no frozen"] and "cavoid_crowd_eval_run" in ev["no frozen"]
    assert "run_fused_crowd" in ac["no frozen"] and "cavoid_crowd_actor_run" in ac["no frozen"]
    with pytest.raises(ValueError):
        why_actor(65, 0, "rnn", ("split", 16), 19, 19, "rnn")


def test_the_existing_reasons_and_switches_say_what_they_said_for_frozen_cases():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate, evaluate_fused_crowd_unavailable_reason
    from rl_collision_avoidance_amd.ga3c.rollout import crowd_actor_unavailable_reason, crowd_ws_actor_unavailable_reason
    assert crowd_actor_unavailable_reason(20, 0, "rnn", ("split", 16), 19, 19, True) == (
        "frozen-network agents (the crowd actor kernel carries one network: no _mix form)")
    assert crowd_ws_actor_unavailable_reason(20, 0, "weight_sharing", 19, 19, True) == (
        "frozen-network agents (the crowd weight_sharing actor kernel carries one network: no _mix form)")
    assert evaluate_fused_crowd_unavailable_reason(_env(20, 19), _fused(19), _fused(19)) == (
        "a frozen_policy (the crowd evaluation kernel carries one network: there is no frozen form of this launch)")
    assert evaluate_fused_crowd_unavailable_reason(_env(20, 19), _fused(19)) == (
        "frozen-network agents (the crowd evaluation kernel carries one network; they act by their own)")
    with pytest.raises(ValueError, match=r"evaluate\(fused_crowd=True\) does not apply: a frozen_policy \(the crowd evaluation kernel carries one network"):
        evaluate(_env(20, 19), _fused(19), fused_crowd=True, frozen_policy=_fused(19))


def test_the_five_switches_exclude_each_other_and_raise_with_the_reason():
    import inspect
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate
    assert inspect.signature(evaluate).parameters["fused_crowd_mix"].default is False
    names = ("fused", "fused_ws", "fused_crowd", "fused_crowd_ws", "fused_crowd_mix")
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            with pytest.raises(ValueError, match="exclude"):
                evaluate(_env(20, 19), _fused(19), frozen_policy=_fused(19), **{a: True, b: True})
    with pytest.raises(ValueError, match="exclude"):
        evaluate(_env(20, 19), _fused(19), **{n: True for n in names})
    # fused_crowd_mix=True raises with the reason, before anything touches a device
    with pytest.raises(ValueError, match=r"fused_crowd_mix=True.*FusedPolicy"):
        evaluate(_env(20, 19), lambda x: (x, x), fused_crowd_mix=True, frozen_policy=_fused(19))
    with pytest.raises(ValueError, match=r"fused_crowd_mix=True.*no frozen_policy.*fused_crowd=True"):
        evaluate(_env(20, 19), _fused(19), fused_crowd_mix=True)
    with pytest.raises(ValueError, match=r"fused_crowd_mix=True.*cavoid_eval_run"):
        evaluate(_env(4, 3), _fused(3), fused_crowd_mix=True, frozen_policy=_fused(3))
    with pytest.raises(ValueError, match="steps_per_launch"):
        evaluate(_env(20, 19), _fused(19), fused_crowd_mix=True, frozen_policy=_fused(19), steps_per_launch=0)


def test_train_cli_knows_both_flags(monkeypatch):
    import argparse
    from rl_collision_avoidance_amd.ga3c import train
    seen = {}

    class Stop(Exception):
        pass

    def parse(self, argv=None):
        seen["args"] = argparse.ArgumentParser.parse_known_args(self, argv)[0]
        raise Stop()
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    base = ["--agents", "20", "--scripted-fraction", "0.5", "--frozen-fraction", "0.5"]
    for argv, actor, ev in ((base + ["--fused-crowd-mix-actor"], True, False), (base + ["--evaluate", "1", "--fused-crowd-mix-evaluate"], False, True),
                            (base, False, False)):
        with pytest.raises(Stop):
            train.main(argv)
        assert seen["args"].fused_crowd_mix_actor is actor and seen["args"].fused_crowd_mix_evaluate is ev
        assert seen["args"].fused_crowd_actor is False and seen["args"].fused_crowd_evaluate is False
    monkeypatch.undo()
    src = open(os.path.join(ROOT, "rl_collision_avoidance_amd", "ga3c", "train.py")).read()
    assert '"fused crowd actor kernel (cavoid_crowd_actor_run_mix: learner + frozen network), %d env steps per launch"' in src
    assert '"[Evaluate] fused crowd evaluation kernel (cavoid_crowd_eval_run_mix), %d env steps per launch"' in src
    assert "--fused-crowd-mix-actor: the crowd actor kernel with a frozen network (cavoid_crowd_actor_run_mix) does not apply: " in src
    assert "--fused-crowd-mix-evaluate: the fused crowd evaluation kernel with a frozen network (cavoid_crowd_eval_run_mix)" in src


def test_build_lists_both_units_with_the_licm_flag():
    from rl_collision_avoidance_amd import build
    for name, own in (("cavoid_crowd_actor_mix.hip", "cavoid_crowd_actor_mix.hpp"), ("cavoid_crowd_eval_mix.hip", "cavoid_crowd_eval_mix.hpp")):
        assert [os.path.basename(s) for s in build.SOURCES].count(name) == 1
        assert build.EXTRA_FLAGS[name] == ["-mllvm", "-disable-machine-licm"]
        heads = build.HEADERS[name]
        assert own in heads and all(os.path.exists(os.path.join(build.CSRC, h)) for h in heads)
        assert os.path.join(build.CSRC, own) in build.DEPS                        # (the source digest covers it)
        # every header the unit's own header chain includes by name is listed
        seen, todo = set(), [name]
        while todo:
            f = todo.pop()
            for inc in re.findall(r'#include\s+"(cavoid_\w+\.hpp)"', open(os.path.join(build.CSRC, f)).read()):
                if inc not in seen:
                    seen.add(inc); todo.append(inc)
        assert seen <= set(heads), sorted(seen - set(heads))


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))),
                    reason="llvm-objdump / llvm-readelf of the ROCm toolchain not present")
def test_crowd_mix_kernels_fit_two_workgroups_per_cu_without_scratch():
    """no scratch and at most 256 registers are CONDITIONS of two workgroups of four wavefronts per CU (512 registers per SIMD lane), not
    measurements; the one-network kernels are still four instantiations each"""
    text = _kernel_notes()
    clash = (r"actor_kernel|actor_ws_kernel|eval_kernel|eval_ws_kernel|crowd_kernel|crowd_push_kernel|crowd_rvo_kernel|crowd_rvo_push_kernel|"
             r"crowd_actor_kernel|crowd_evaluate_kernel|crowd_ws_rollout_kernel|crowd_ws_evaluate_kernel|policy_crowd_forward_kernel")
    for kernel in ("crowd_mix_rollout_kernel", "crowd_mix_evaluate_kernel"):
        found = re.findall(r"\.name:\s+(\S*%s\S*)\s*\n\s*\.private_segment_fixed_size:\s+(\d+)" % kernel, text)
        assert len(found) == 4, found                                             # two buckets of the agent count (32, 64) x (plain, ORCA-carrying env step)
        want = sorted((nb, r) for nb in ("32", "64") for r in "01")
        assert sorted(re.search(r"%sILi(\d+)ELb(\d)E" % kernel, name).groups() for name, _ in found) == want
        assert all(int(size) == 0 for _, size in found), found
        sizes = re.findall(r"\.max_flat_workgroup_size:\s+(\d+)\s*\n\s*\.name:\s+\S*%s" % kernel, text)
        assert sizes == ["256"] * 4, sizes
        vgprs = re.findall(r"\.name:\s+\S*%s\S*\s*\n(?:\s+\.(?!name)\S+:.*\n)*?\s+\.vgpr_count:\s+(\d+)" % kernel, text)
        assert len(vgprs) == 4 and all(int(v) <= 256 for v in vgprs), vgprs
        assert not any(re.search(clash, name) for name, _ in found), found        # clear of the substrings other tests count kernels by
    for kernel in ("crowd_actor_kernel", "crowd_evaluate_kernel"):
        found = re.findall(r"\.name:\s+(\S*%s\S*)\s*\n\s*\.private_segment_fixed_size:\s+(\d+)" % kernel, text)
        assert len(found) == 4 and all(int(size) == 0 for _, size in found), found
