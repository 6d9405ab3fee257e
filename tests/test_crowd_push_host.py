"""CPU tests of `cavoid_step_push` on crowd worlds: which launches `BatchedRollout.step` takes (the pure function behind
`BatchedRollout.step_path`) and the built library's `crowd_push_kernel` instantiations (two buckets, zero scratch)."""
import os
import re

import pytest

from tests.host_support import LLVM, _kernel_notes

ONE, THREE = "step_push", "env, push, episode log"


def test_step_path_is_one_launch_for_every_agent_count_with_table_actions():
    # The default follows a measurement (tools/crowdpushbench.py: the one launch must not be slower than the three at 20 x 2048,
    # 32 x 1024 or 64 x 512 by more than a repeat's spread).  profiles/crowd_step_push_timing.txt: it takes 0.63, 0.64 and 0.56 of the
    # three launches' time, so 17..64 agents take it by default as 1..16 do.
    from rl_collision_avoidance_amd.ga3c.rollout import step_path
    for n in range(1, 65):
        for dyn in (0, 1):
            assert step_path(n, dyn, True) == ONE, (n, dyn)


def test_step_path_keeps_three_launches_for_velocity_actions_and_when_switched_off():
    from rl_collision_avoidance_amd.ga3c.rollout import step_path
    for n in (1, 4, 16, 17, 20, 33, 64):
        assert step_path(n, 2, True) == THREE, n             # holonomic dynamics: cavoid_step_push takes table actions only
        for dyn in (0, 1, 2):
            assert step_path(n, dyn, False) == THREE, (n, dyn)   # CAVOID_FUSE_ENV_PUSH=0
    for n in (0, 65):
        with pytest.raises(ValueError):
            step_path(n, 0, True)


def test_rollout_has_a_read_only_step_path():
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    prop = BatchedRollout.__dict__["step_path"]
    assert isinstance(prop, property) and prop.fset is None

    class Cfg:
        dynamics = 0

    class Env:
        max_agents, cfg = 20, Cfg()
    roll = BatchedRollout.__new__(BatchedRollout)            # (no device here: the property reads three host values)
    roll.env, roll.fuse_env_push, roll._h = Env(), True, None
    assert roll.step_path == ONE                             # 20 agents per world: the crowd form's one launch
    roll.fuse_env_push = False
    assert roll.step_path == THREE
    roll.fuse_env_push, Env.cfg.dynamics = True, 2
    assert roll.step_path == THREE


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))),
                    reason="llvm-objdump / llvm-readelf of the ROCm toolchain not present")
def test_crowd_push_kernels_use_no_scratch():
    text = _kernel_notes()
    found = re.findall(r"\.name:\s+(\S*crowd_push_kernel\S*)\s*\n\s*\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(found) == 2, found            # two buckets of the agent count (32, 64)
    assert all(int(size) == 0 for _, size in found), found
    # a workgroup of two wavefronts: the env step and bookkeeping on one, the row copy on the other
    sizes = re.findall(r"\.max_flat_workgroup_size:\s+(\d+)\s*\n\s*\.name:\s+\S*crowd_push_kernel", text)
    assert sizes == ["128", "128"], sizes
