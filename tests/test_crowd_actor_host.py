"""CPU tests of the crowd worlds' fused actor loop (`cavoid_crowd_actor_run`, csrc/cavoid_crowd_actor.hpp): the exported symbol and its
argument check, the pure function that says when `BatchedRollout.run_fused_crowd` applies, what stays as it was for the default paths, the
training CLI's flag, and the built library's four `crowd_actor_kernel` instantiations (zero scratch, 256 threads)."""
import ctypes as C
import os
import re

import pytest

from tests.host_support import LLVM, ROOT, _kernel_notes

DEFAULT_FORM = ("split", 16)


def test_library_exports_the_entry_point_and_checks_its_arguments():
    from rl_collision_avoidance_amd import _lib
    header = open(os.path.join(ROOT, "include", "cavoid.h")).read()
    assert re.search(r"\bint\s+cavoid_crowd_actor_run\s*\(", header)
    assert re.search(r"#define\s+CAVOID_ABI_VERSION\s+3\b", header)              # additive: the version stays
    assert any(name == "cavoid_crowd_actor_run" for name, _, _ in _lib.SYMBOLS)
    fn = _lib.lib().cavoid_crowd_actor_run                                        # (AttributeError if the library lacks it)
    # cavoid_actor_run's argument list
    assert [s for s in _lib.SYMBOLS if s[0] == "cavoid_crowd_actor_run"][0][1:] == [s for s in _lib.SYMBOLS if s[0] == "cavoid_actor_run"][0][1:]
    assert fn(None, None, None, None, None, None, None, None, None, None, None, 2, 0, None) == -1      # CAVOID_EINVAL
    b = _lib.CavoidRolloutBuffers()
    b.struct_size = C.sizeof(_lib.CavoidRolloutBuffers)
    assert fn(None, None, None, C.byref(b), None, None, None, None, None, None, None, 0, 0, None) == -1   # ... before n_steps == 0 is looked at


def test_reason_is_none_for_what_the_kernel_carries():
    from rl_collision_avoidance_amd.ga3c.rollout import crowd_actor_unavailable_reason as why
    for n in range(17, 65):
        for dyn in (0, 1):
            for m in (1, 16, 19, 20, 23, 24, n - 1):
                assert why(n, dyn, "rnn", DEFAULT_FORM, m, m, False) is None, (n, dyn, m)


def test_reason_names_each_refusal():
    from rl_collision_avoidance_amd.ga3c.rollout import crowd_actor_unavailable_reason as why
    for n in (1, 4, 16):
        assert "run_fused" in why(n, 0, "rnn", DEFAULT_FORM, n - 1, n - 1, False) and "16" in why(n, 0, "rnn", DEFAULT_FORM, n - 1, n - 1, False)
    assert "weight_sharing" in why(20, 0, "weight_sharing", ("f32", 0), 7, 7, False)
    assert "holonomic" in why(20, 2, "rnn", DEFAULT_FORM, 19, 19, False)
    for form in (("split", 3), ("split", 4), ("f32", 0)):
        assert "non-default inference form" in why(33, 0, "rnn", form, 32, 32, False)
    assert "frozen-network agents" in why(20, 0, "rnn", DEFAULT_FORM, 19, 19, True)
    r = why(20, 0, "rnn", DEFAULT_FORM, 10, 19, False)
    assert "10" in r and "19" in r and "neighbours" in r
    assert "FusedPolicy" in why(20, 0, "rnn", DEFAULT_FORM, 19, 19, False, fused_policy=False)
    for n in (0, 65):
        with pytest.raises(ValueError):
            why(n, 0, "rnn", DEFAULT_FORM, 3, 3, False)


def _bare_rollout(n, m, policy):
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout

    class Cfg:
        dynamics, max_other, rvo_enabled, max_agents, gen_frozen_fraction, gen_nonlearning_fraction = 0, m, 0, n, 0.0, 0.0

    class Env:
        max_agents, cfg = n, Cfg()
    roll = BatchedRollout.__new__(BatchedRollout)            # (no device here: the properties read host values)
    roll.env, roll.policy, roll.frozen_policy, roll.fuse_env_push, roll._h = Env(), policy, None, True, None
    return roll


class _Fused:
    accepts_strided_obs, arch, inference_form = True, "rnn", DEFAULT_FORM

    def __init__(self, m):
        self.max_others = m


def test_the_default_paths_say_what_they_said():
    roll = _bare_rollout(20, 19, _Fused(19))
    assert roll.fused_unavailable_reason == "more than 16 agents per world (the crowd step form has no fused actor kernel)"
    assert not roll.fused_available
    assert roll.actor_path == ("one launch per phase (policy, env + bookkeeping) -- fused kernel not applicable: more than 16 agents per world "
                               "(the crowd step form has no fused actor kernel)")
    # ... while the opt-in form applies, and says why where it does not
    assert roll.crowd_fused_unavailable_reason is None and roll.crowd_fused_available
    assert "neighbours" in _bare_rollout(20, 19, _Fused(7)).crowd_fused_unavailable_reason
    tile = _bare_rollout(4, 3, _Fused(3))
    assert tile.fused_available and not tile.crowd_fused_available
    with pytest.raises(RuntimeError, match="run_fused"):
        tile.run_fused_crowd(2)                              # (refused before anything touches a device)


def test_train_cli_knows_the_flag(monkeypatch):
    """the parser accepts --fused-crowd-actor (off by default); parsing stops before anything touches a device"""
    import argparse
    from rl_collision_avoidance_amd.ga3c import train
    seen = {}

    class Stop(Exception):
        pass

    def parse(self, argv=None):
        seen["args"] = argparse.ArgumentParser.parse_known_args(self, argv)[0]
        raise Stop()
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    for argv, want in ((["--fused-crowd-actor"], True), ([], False)):
        with pytest.raises(Stop):
            train.main(argv)
        assert seen["args"].fused_crowd_actor is want and seen["args"].no_actor_kernel is False
    monkeypatch.undo()
    with pytest.raises(SystemExit):                          # (an unknown flag is still an error)
        train.main(["--fused-crowd-actor-typo"])


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))),
                    reason="llvm-objdump / llvm-readelf of the ROCm toolchain not present")
def test_crowd_actor_kernels_use_no_scratch():
    text = _kernel_notes()
    found = re.findall(r"\.name:\s+(\S*crowd_actor_kernel\S*)\s*\n\s*\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(found) == 4, found            # two buckets of the agent count (32, 64) x (plain, ORCA-carrying env step)
    assert all(int(size) == 0 for _, size in found), found
    assert sorted(re.search(r"crowd_actor_kernelILi(\d+)ELb(\d)E", name).groups() for name, _ in found) == [("32", "0"), ("32", "1"), ("64", "0"), ("64", "1")]
    # one workgroup of four wavefronts per crowd tile
    sizes = re.findall(r"\.max_flat_workgroup_size:\s+(\d+)\s*\n\s*\.name:\s+\S*crowd_actor_kernel", text)
    assert sizes == ["256"] * 4, sizes
    # the names stay clear of the substrings other tests count kernels by
    assert not any(re.search(r"crowd_kernel|crowd_push_kernel|crowd_rvo_kernel|policy_crowd_forward_kernel", name) for name, _ in found)
