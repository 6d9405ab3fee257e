"""CPU tests of the fused evaluation loop (`cavoid_eval_run`, csrc/cavoid_eval.hpp; `ga3c.evaluate(fused=True)`): the exported symbol and
its argument check, the record struct's layout, the training CLI's flag, the reduction from records to the result dict held against
hand-made records, the reasons the kernel does not apply that need no device, and the built kernels' registers and scratch."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests.host_support import LLVM, ROOT, _kernel_notes

DEFAULT_FORM = ("split", 16)


def test_library_exports_the_entry_point_and_checks_its_arguments():
    from rl_collision_avoidance_amd import _lib
    header = open(os.path.join(ROOT, "include", "cavoid.h")).read()
    assert re.search(r"\bint\s+cavoid_eval_run\s*\(", header)
    assert re.search(r"#define\s+CAVOID_ABI_VERSION\s+3\b", header)              # additive: the version stays
    assert "An agent's return sums the rewards up to and including the step at which its world is over." in header
    assert any(name == "cavoid_eval_run" for name, _, _ in _lib.SYMBOLS)
    fn = _lib.lib().cavoid_eval_run                                               # (AttributeError if the library lacks it)
    assert fn(None, None, None, None, None, None, None, None, None, None, 2, 1, None) == -1       # CAVOID_EINVAL
    b = _lib.CavoidEvalBuffers()
    b.struct_size = C.sizeof(_lib.CavoidEvalBuffers)
    assert fn(None, None, None, C.byref(b), None, None, None, None, None, None, 0, 1, None) == -1  # ... before n_steps == 0 is looked at


def test_record_struct_mirrors_the_header():
    from rl_collision_avoidance_amd import _lib
    header = open(os.path.join(ROOT, "include", "cavoid.h")).read()
    body = re.search(r"typedef struct cavoid_eval_buffers \{(.*?)\} cavoid_eval_buffers;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|double|float)\s*(\*?)\s*(\w+)\s*;", body)
    assert [name for _, _, name in fields] == [name for name, _ in _lib.CavoidEvalBuffers._fields_]
    assert [name for name, _ in _lib.CavoidEvalBuffers._fields_] == ["struct_size", "ret", "goal_step", "world_steps", "worlds_running"]
    for (ctype, star, name), (_, py) in zip(fields, _lib.CavoidEvalBuffers._fields_):
        assert py is (C.c_void_p if star else C.c_int32), name
    assert fields[1][0] == "double" and all(f[0] == "int32_t" for f in fields[2:])
    # int32 + padding + four pointers, as the C compiler lays it out
    assert C.sizeof(_lib.CavoidEvalBuffers) == 8 + 4 * C.sizeof(C.c_void_p)
    assert _lib.CavoidEvalBuffers.ret.offset == 8


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
    for argv, want in ((["--evaluate", "1", "--fused-evaluate"], True), (["--evaluate", "1"], False)):
        with pytest.raises(Stop):
            train.main(argv)
        assert seen["args"].fused_evaluate is want
    monkeypatch.undo()
    src = open(os.path.join(ROOT, "rl_collision_avoidance_amd", "ga3c", "train.py")).read()
    assert '"[Evaluate] fused evaluation kernel (cavoid_eval_run), %d env steps per launch"' in src


# ---- the reduction, on hand-made records --------------------------------------------------------------------------------------------
GOAL, OUT, COLL, WAS_GOAL, WAS_COLL, PRESENT, LEARNING = 1, 2, 4, 8, 16, 32, 64
DT, NEAR = 0.2, 0.5


def _round(rows, env_steps):
    """rows: (start x, goal x, preferred speed, flags at reset, flags at the end, goal_step, return) per agent, all on the x axis"""
    A = len(rows)
    f64 = torch.zeros(4, A, dtype=torch.float64)
    f32 = torch.zeros(5, A, dtype=torch.float32)
    for k, (x0, gx, pref, _, _, _, _) in enumerate(rows):
        f64[0, k], f32[0, k], f32[3, k] = x0, gx, pref
    return {"ret": torch.tensor([r[6] for r in rows], dtype=torch.float64), "goal_step": torch.tensor([r[5] for r in rows], dtype=torch.int32),
            "env_steps": env_steps, "state0": (f64, f32, torch.tensor([r[3] for r in rows], dtype=torch.int32)),
            "flags_end": torch.tensor([r[4] for r in rows], dtype=torch.int32)}


def test_reduction_on_known_records():
    from rl_collision_avoidance_amd.ga3c.evaluate import (OUTCOME_COLLISION, OUTCOME_GOAL, OUTCOME_TIMEOUT, OUTCOME_UNFINISHED,
                                                         reduce_outcomes)
    L = PRESENT | LEARNING
    rows = [
        (0.0, 4.5, 1.0, L, L | GOAL, 25, 1.0),                    # goal: 25 steps = 5.0 s, straight line (4.5 - 0.5) / 1.0 = 4.0 s -> 1.0 s extra
        (0.0, 3.0, 1.0, L, L | COLL | WAS_COLL, 0, -0.25),        # collision
        (0.0, 3.0, 1.0, L, L | OUT, 0, -0.5),                     # timeout
        (0.0, 3.0, 1.0, L, L, 0, 0.125),                          # unfinished (the round hit max_steps)
        (0.0, 2.5, 2.0, L, L | GOAL | COLL, 10, 0.75),            # goal AND collision flag: counts as goal; 2.0 s, straight 1.0 s -> 1.0 s extra
        (0.0, 3.0, 1.0, PRESENT, PRESENT | GOAL, 7, 100.0),       # a scripted agent: in per_agent, not in the rates
        (0.0, 3.0, 1.0, 0, 0, 0, 0.0),                            # an empty slot
    ]
    res = reduce_outcomes([_round(rows, 40)], DT, NEAR, details=True)
    assert res["agents"] == 5 and res["env_steps"] == 40
    assert res["success_rate"] == 2 / 5 and res["collision_rate"] == 1 / 5 and res["timeout_rate"] == 1 / 5
    assert res["unfinished_rate"] == pytest.approx(1 / 5, abs=1e-15)
    assert res["mean_reward"] == (1.0 - 0.25 - 0.5 + 0.125 + 0.75) / 5
    assert res["mean_time_to_goal"] == (25 * DT + 10 * DT) / 2
    assert res["mean_extra_time_to_goal"] == ((25 * DT - 4.0) + (10 * DT - 1.0)) / 2
    per = res["per_agent"]
    assert per["outcome"].tolist() == [OUTCOME_GOAL, OUTCOME_COLLISION, OUTCOME_TIMEOUT, OUTCOME_UNFINISHED, OUTCOME_GOAL, OUTCOME_GOAL, OUTCOME_UNFINISHED]
    assert per["learning"].tolist() == [True] * 5 + [False] * 2
    assert per["time_to_goal"].tolist() == [25 * DT, 0.0, 0.0, 0.0, 10 * DT, 7 * DT, 0.0]
    assert per["extra_time"].tolist()[:5] == [25 * DT - 4.0, 0.0, 0.0, 0.0, 10 * DT - 1.0]
    assert per["ret"].tolist() == [r[6] for r in rows] and per["ret"].dtype == torch.float64
    # without details: today's keys, nothing else
    plain = reduce_outcomes([_round(rows, 40)], DT, NEAR)
    assert list(plain) == ["agents", "success_rate", "collision_rate", "timeout_rate", "unfinished_rate", "mean_reward", "mean_time_to_goal",
                           "mean_extra_time_to_goal", "env_steps"]
    assert all(plain[k] == res[k] for k in plain)
    # two rounds add up
    two = reduce_outcomes([_round(rows, 40), _round(rows[:3], 9)], DT, NEAR, details=True)
    assert two["agents"] == 8 and two["env_steps"] == 49 and two["success_rate"] == 3 / 8 and two["per_agent"]["ret"].numel() == 10


def test_percentiles_of_a_five_value_list():
    from rl_collision_avoidance_amd.ga3c.evaluate import reduce_outcomes
    L = PRESENT | LEARNING
    # extra times 1, 2, 3, 4, 5 s (straight line 4.0 s at 1 m/s), handed over out of order
    rows = [(0.0, 4.5, 1.0, L, L | GOAL, int(round((4.0 + e) / DT)), 0.0) for e in (3.0, 1.0, 5.0, 2.0, 4.0)]
    res = reduce_outcomes([_round(rows, 50)], DT, NEAR, details=True)
    assert res["extra_time_p75"] == pytest.approx(4.0, abs=1e-12)                # numpy.percentile([1..5], 75)
    assert res["extra_time_p90"] == pytest.approx(4.6, abs=1e-12)                # numpy.percentile([1..5], 90)
    assert res["mean_extra_time_to_goal"] == pytest.approx(3.0, abs=1e-12)
    # nobody reached the goal: zeros, like the means
    none = reduce_outcomes([_round([(0.0, 3.0, 1.0, L, L | OUT, 0, 0.0)], 5)], DT, NEAR, details=True)
    assert none["extra_time_p75"] == 0.0 and none["extra_time_p90"] == 0.0 and none["mean_time_to_goal"] == 0.0


def test_goal_step_zero_never_enters_the_time_sums():
    from rl_collision_avoidance_amd.ga3c.evaluate import reduce_outcomes
    L = PRESENT | LEARNING
    rows = [(0.0, 4.5, 1.0, L, L | GOAL, 25, 0.0),
            (0.0, 9.0, 1.0, L, L | GOAL, 0, 0.0)]                 # the flag without a recorded step: a goal in the rates, no time
    res = reduce_outcomes([_round(rows, 30)], DT, NEAR, details=True)
    assert res["success_rate"] == 1.0
    assert res["mean_time_to_goal"] == (25 * DT) / 2 and res["mean_extra_time_to_goal"] == (25 * DT - 4.0) / 2   # (no -8.5 s from the second)
    assert res["per_agent"]["time_to_goal"].tolist() == [25 * DT, 0.0] and res["per_agent"]["extra_time"].tolist() == [25 * DT - 4.0, 0.0]
    assert res["extra_time_p75"] == pytest.approx(1.0) and res["extra_time_p90"] == pytest.approx(1.0)


# ---- the reasons that need no device ------------------------------------------------------------------------------------------------
def _env(n, m=None, dynamics=0, frozen=0.0, nonlearning=0.0, rvo=0):
    m = n - 1 if m is None else m
    cfg = SimpleNamespace(dynamics=dynamics, gen_frozen_fraction=frozen, gen_nonlearning_fraction=nonlearning, rvo_enabled=rvo)
    return SimpleNamespace(max_agents=n, max_other=m, cfg=cfg)


def _fused(m, arch="rnn", form=DEFAULT_FORM):
    return SimpleNamespace(act=lambda *a, **k: None, inference_form=form, _h=object(), arch=arch, ws=arch == "weight_sharing", max_others=m)


def test_reasons_without_a_device():
    from rl_collision_avoidance_amd.ga3c.evaluate import evaluate, evaluate_fused_unavailable_reason as why
    for n in (1, 2, 4, 10, 16):
        assert why(_env(n, max(n - 1, 1)), _fused(max(n - 1, 1))) is None
    assert why(_env(4, 3, rvo=1, nonlearning=0.5), _fused(3)) is None
    assert why(_env(4, 3, frozen=0.3, nonlearning=0.5), _fused(3), _fused(3)) is None
    r = why(_env(20, 19), _fused(19))                        # a crowd env config
    assert "crowd" in r and "20" in r and "16" in r
    assert "weight_sharing" in why(_env(4, 3), _fused(3, arch="weight_sharing", form=("f32", 0)))
    assert "weight_sharing" in why(_env(4, 3), _fused(3), _fused(3, arch="weight_sharing", form=("f32", 0)))
    assert "FusedPolicy" in why(_env(4, 3), lambda x: (x, x))    # a plain callable policy
    assert "19" in why(_env(16, 24), _fused(24))
    assert "holonomic" in why(_env(4, 3, dynamics=2), _fused(3))
    assert "non-default inference form" in why(_env(4, 3), _fused(3, form=("split", 3)))
    assert "frozen" in why(_env(4, 3, frozen=0.3, nonlearning=0.5), _fused(3))
    r = why(_env(4, 3), _fused(2))
    assert "2" in r and "3" in r and "neighbours" in r
    assert "ORCA" in why(_env(16, 15, rvo=1), _fused(15))
    with pytest.raises(ValueError, match="FusedPolicy"):         # fused=True raises with the reason, before anything touches a device
        evaluate(_env(4, 3), lambda x: (x, x), fused=True)


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))),
                    reason="llvm-objdump / llvm-readelf of the ROCm toolchain not present")
def test_eval_kernels_take_no_scratch_and_no_more_registers_than_the_actor():
    text = _kernel_notes()
    pat = r"\.name:\s+\S*%sILi(\d+)ELb(\d)ELb(\d)E\S*\s*\n\s*\.private_segment_fixed_size:\s+(\d+)"
    found = {k[:3]: int(k[3]) for k in re.findall(pat % "eval_kernel", text)}
    assert len(found) == 48, sorted(found)                   # 1..16 agents x (plain, ORCA, ORCA + frozen network)
    assert found[("4", "0", "0")] == 0 and found[("10", "0", "0")] == 0
    vg = r"\.name:\s+\S*%sILi(\d+)ELb(\d)ELb(\d)E\S*\s*\n(?:\s+\.(?!name)\S+:.*\n)*?\s+\.vgpr_count:\s+(\d+)"
    ev = {k[:3]: int(k[3]) for k in re.findall(vg % "eval_kernel", text)}
    ac = {k[:3]: int(k[3]) for k in re.findall(vg % "actor_kernel", text)}
    assert len(ev) == 48 and len(ac) == 48
    for n in ("4", "10"):
        assert ev[(n, "0", "0")] <= ac[(n, "0", "0")], (n, ev[(n, "0", "0")], ac[(n, "0", "0")])
    sizes = re.findall(r"\.max_flat_workgroup_size:\s+(\d+)\s*\n\s*\.name:\s+\S*eval_kernel", text)
    assert sizes == ["256"] * 48, sizes
