"""CPU tests of the crowd worlds' fused actor loop for the weight_sharing network (`cavoid_crowd_actor_run_ws`,
csrc/cavoid_crowd_actor_ws.hpp): `crowd_ws_actor_unavailable_reason` -- the pure function behind
`BatchedRollout.crowd_ws_fused_unavailable_reason` and `ga3c.train --fused-crowd-ws-actor` -- against the refusals the C entry point
documents, the entry point's declaration, export and binding, what stays as it was for the other paths, the training CLI's flag, and the
built library's four `crowd_ws_rollout_kernel` instantiations (zero scratch, 256 threads, within 256 registers)."""
import os
import re

import pytest

from tests.host_support import LLVM, ROOT, _kernel_notes

CSRC = os.path.join(ROOT, "rl_collision_avoidance_amd", "csrc")


def _reason(**over):
    from rl_collision_avoidance_amd.ga3c.rollout import crowd_ws_actor_unavailable_reason
    # WS-8 in a 20-agent world
    kw = dict(agents_per_world=20, dynamics=0, arch="weight_sharing", policy_max_others=7, env_max_other=7, frozen_agents=False,
              env_step_lds=20000, fused_policy=True)
    kw.update(over)
    return crowd_ws_actor_unavailable_reason(**kw)


def test_reason_is_none_for_what_the_kernel_carries():
    from rl_collision_avoidance_amd.ga3c import rollout
    for n in range(17, 65):
        for m in (1, 7, 19, 20, 63):
            for dyn in (0, 1):
                # the LDS of the crowd env step at this shape: always inside the loan (cavoid_create refuses a crowd env above 64 KiB)
                lds = rollout.crowd_env_step_lds_bytes(n, 6 + 7 * m)
                assert lds <= 65536 < rollout.WS_ACTOR_LENT_BYTES, (n, m, lds)
                assert _reason(agents_per_world=n, dynamics=dyn, policy_max_others=m, env_max_other=m, env_step_lds=lds) is None, (n, m, dyn)


@pytest.mark.parametrize("over,words", [
    (dict(agents_per_world=16), ("run_fused_ws", "16 agents per world")),
    (dict(agents_per_world=4), ("run_fused_ws", "cavoid_actor_run_ws")),
    (dict(arch="rnn"), ("rnn network", "run_fused_crowd")),
    (dict(dynamics=2), ("holonomic",)),
    (dict(frozen_agents=True), ("frozen-network agents",)),
    (dict(policy_max_others=3), ("observes 3 neighbours", "the env's rows carry 7")),
    (dict(env_step_lds=65540), ("does not fit", "65536")),
    (dict(fused_policy=False), ("not a FusedPolicy",)),
    # above 19 observed neighbours the policy is a FusedPolicy only on the ring kernels: the reason says how to get one
    (dict(fused_policy=False, policy_max_others=-1, env_max_other=20), ("not a FusedPolicy", "--fused-crowd-ws", "ws_crowd=True")),
])
def test_each_refusal_names_its_cause(over, words):
    why = _reason(**over)
    assert why is not None and all(w in why for w in words), why


def test_the_plain_not_a_fused_policy_reason_does_not_send_narrow_rows_to_the_ring_flag():
    assert "--fused-crowd-ws" not in _reason(fused_policy=False, env_max_other=19)


def test_agent_count_out_of_range_is_an_error():
    for n in (0, 65):
        with pytest.raises(ValueError):
            _reason(agents_per_world=n)


def test_the_env_step_bound_is_the_crowd_kernels_allocation():
    """`crowd_env_step_lds_bytes` mirrors crowd_actor_env_lds_bytes at the tile cavoid_create chooses: spot values worked out from
    cavoid_crowd.hpp by hand (StageRec is 8 floats; lds_floats_block 128; lds_floats_scratch 576)."""
    from rl_collision_avoidance_amd.ga3c import rollout
    # n = 20, M = 7: width 55; fixed 512 + 256 + 576 + 19 * 80 = 2864; keys 19 * 128 = 2432; rows (2432 // 57) & ~3 = 40 -> 2200 floats < keys
    assert rollout.crowd_env_step_lds_bytes(20, 55) == 4 * (128 + 2864 + 2432)
    # n = 64, M = 63: width 447; fixed 1344 + 63 * 80 = 6384; keys 8064; rows (8064 // 449) & ~3 = 16 -> 7152 floats < keys
    assert rollout.crowd_env_step_lds_bytes(64, 447) == 4 * (128 + 6384 + 8064)
    # n = 17, M = 63 (a padded row): keys 2048; rows (2048 // 449) & ~3 = 4 -> 1788 floats < keys
    assert rollout.crowd_env_step_lds_bytes(17, 447) == 4 * (128 + 1344 + 16 * 80 + 2048)
    # the bound stands once, in the crowd launches' shared prologue, and this unit hands it the weight_sharing loan
    helper = open(os.path.join(CSRC, "cavoid_loop_host.hpp")).read()
    assert re.search(r"lds\s*>\s*65536\s*\|\|\s*lds\s*>\s*lent\b", helper)
    src = open(os.path.join(CSRC, "cavoid_crowd_actor_ws.hip")).read()
    assert re.search(r"crowd_loop_tiles\(\s*e\s*,\s*(?:/\*lent=\*/\s*)?actor_ws_lent_bytes\(\)\s*,", src)


def test_the_entry_point_is_declared_exported_and_bound():
    from rl_collision_avoidance_amd import _lib
    header = open(os.path.join(ROOT, "include", "cavoid.h")).read()
    assert re.search(r"\bint\s+cavoid_crowd_actor_run_ws\s*\(", header)
    assert re.search(r"#define\s+CAVOID_ABI_VERSION\s+3\b", header)              # additive: the version stays
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert "cavoid_crowd_actor_run_ws" in bound and len(bound["cavoid_crowd_actor_run_ws"][1]) == 14
    assert bound["cavoid_crowd_actor_run_ws"] == bound["cavoid_actor_run_ws"] == bound["cavoid_crowd_actor_run"]
    fn = _lib.lib().cavoid_crowd_actor_run_ws                                     # (AttributeError if the library lacks it)
    assert fn(None, None, None, None, None, None, None, None, None, None, None, 2, 0, None) == -1      # CAVOID_EINVAL
    import ctypes as C
    b = _lib.CavoidRolloutBuffers()
    b.struct_size = C.sizeof(_lib.CavoidRolloutBuffers)
    assert fn(None, None, None, C.byref(b), None, None, None, None, None, None, None, 0, 0, None) == -1   # ... before n_steps == 0 is looked at


def test_the_unit_is_built_like_every_step_loop_unit():
    from rl_collision_avoidance_amd import build
    name = "cavoid_crowd_actor_ws.hip"
    assert [os.path.basename(s) for s in build.SOURCES].count(name) == 1
    assert build.EXTRA_FLAGS[name] == ["-mllvm", "-disable-machine-licm"]
    # every header the unit reaches is in its dependency list
    seen, todo = set(), [name]
    while todo:
        for inc in re.findall(r'#include\s+"(cavoid_[^"]+\.hpp)"', open(os.path.join(CSRC, todo.pop())).read()):
            if inc not in seen:
                seen.add(inc); todo.append(inc)
    assert seen <= set(build.HEADERS[name]), sorted(seen - set(build.HEADERS[name]))
    # the fused phase and the ring are no longer kept apart, the trainer's pass still is
    ws = open(os.path.join(CSRC, "cavoid_policy_ws.hpp")).read()
    assert re.search(r"static_assert\(!FUSED \|\| !TRAIN,", ws) and "!TRAIN && !Ring::on" not in ws
    hpp = open(os.path.join(CSRC, "cavoid_crowd_actor_ws.hpp")).read()
    assert "policy_ws_forward_tile<false, kLossA3C, PolRing<kWsRing>, true>" in hpp and "__launch_bounds__(256, 2) crowd_ws_rollout_kernel" in hpp


def _bare_rollout(n, m, policy):
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout

    class Cfg:
        dynamics, max_other, rvo_enabled, max_agents, gen_frozen_fraction, gen_nonlearning_fraction = 0, m, 0, n, 0.0, 0.0

    class Env:
        max_agents, cfg, obs_width = n, Cfg(), 6 + 7 * m
    roll = BatchedRollout.__new__(BatchedRollout)            # (no device here: the properties read host values)
    roll.env, roll.policy, roll.frozen_policy, roll.fuse_env_push, roll._h = Env(), policy, None, True, None
    return roll


class _Ws:
    accepts_strided_obs, arch, ws, inference_form = True, "weight_sharing", True, ("f32", 0)

    def __init__(self, m, crowd=False):
        self.max_others, self.crowd = m, crowd


def test_the_rollout_has_the_new_forms_and_the_old_ones_say_what_they_said():
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    for name in ("crowd_ws_fused_unavailable_reason", "crowd_ws_fused_available", "run_fused_crowd_ws", "capture_fused_crowd_ws",
                 "fused_available", "crowd_fused_available", "run_fused_crowd", "ws_fused_available", "run_fused_ws", "actor_path", "step_path"):
        assert hasattr(BatchedRollout, name), name
    for m, crowd in ((7, False), (19, False), (20, True), (63, True)):
        roll = _bare_rollout(64 if m == 63 else 21, m, _Ws(m, crowd))
        assert roll.crowd_ws_fused_unavailable_reason is None and roll.crowd_ws_fused_available
        # ... and the other forms still refuse a weight_sharing policy on a crowd env, in today's words
        assert roll.fused_unavailable_reason == "more than 16 agents per world (the crowd step form has no fused actor kernel)"
        assert not roll.fused_available and "fused kernel not applicable" in roll.actor_path and roll.step_path == "step_push"
        assert "weight_sharing" in roll.crowd_fused_unavailable_reason and not roll.crowd_fused_available
        assert ("ring" if crowd else "crowd worlds") in roll.ws_fused_unavailable_reason and not roll.ws_fused_available
        with pytest.raises(RuntimeError, match="weight_sharing"):
            roll.run_fused_crowd(2)                          # (refused before anything touches a device)
        with pytest.raises(RuntimeError, match="ring" if crowd else "crowd worlds"):
            roll.run_fused_ws(2)
    tile = _bare_rollout(4, 7, _Ws(7))
    assert tile.ws_fused_available and not tile.crowd_ws_fused_available
    with pytest.raises(RuntimeError, match="run_fused_ws"):
        tile.run_fused_crowd_ws(2)
    assert "neighbours" in _bare_rollout(20, 19, _Ws(7)).crowd_ws_fused_unavailable_reason


def test_train_cli_knows_the_flag(monkeypatch):
    """the parser accepts --fused-crowd-ws-actor (off by default); parsing stops before anything touches a device"""
    import argparse
    from rl_collision_avoidance_amd.ga3c import train
    seen = {}

    class Stop(Exception):
        pass

    def parse(self, argv=None):
        seen["args"] = argparse.ArgumentParser.parse_known_args(self, argv)[0]
        raise Stop()
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    for argv, want in ((["--fused-crowd-ws-actor"], True), ([], False)):
        with pytest.raises(Stop):
            train.main(argv)
        assert seen["args"].fused_crowd_ws_actor is want
        assert seen["args"].fused_crowd_actor is False and seen["args"].fused_ws_actor is False and seen["args"].no_actor_kernel is False
    monkeypatch.undo()
    with pytest.raises(SystemExit):                          # (an unknown flag is still an error)
        train.main(["--fused-crowd-ws-actor-typo"])
    src = open(os.path.join(ROOT, "rl_collision_avoidance_amd", "ga3c", "train.py")).read()
    assert "fused crowd weight_sharing actor kernel (cavoid_crowd_actor_run_ws), %d env steps per launch" in src
    assert '"--fused-crowd-ws-actor: the crowd weight_sharing actor kernel (cavoid_crowd_actor_run_ws) does not apply: " + why' in src


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))),
                    reason="llvm-objdump / llvm-readelf of the ROCm toolchain not present")
def test_crowd_ws_rollout_kernels_fit_two_workgroups_per_cu_without_scratch():
    text = _kernel_notes()
    found = re.findall(r"\.name:\s+(\S*crowd_ws_rollout_kernel\S*)\s*\n\s*\.private_segment_fixed_size:\s+(\d+)", text)
    # one ring instantiation of the pass for every neighbour count: two buckets of the agent count (32, 64) x (plain, ORCA-carrying env step)
    assert len(found) == 4, found
    assert sorted(re.search(r"crowd_ws_rollout_kernelILi(\d+)ELb(\d)E", name).groups() for name, _ in found) == [("32", "0"), ("32", "1"), ("64", "0"), ("64", "1")]
    assert all(int(size) == 0 for _, size in found), found
    sizes = re.findall(r"\.max_flat_workgroup_size:\s+(\d+)\s*\n\s*\.name:\s+\S*crowd_ws_rollout_kernel", text)
    assert sizes == ["256"] * 4, sizes
    vgprs = re.findall(r"\.name:\s+\S*crowd_ws_rollout_kernel\S*\s*\n(?:\s+\.(?!name)\S+:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text)
    assert len(vgprs) == 4 and all(int(v) <= 256 for v in vgprs), vgprs
    # the names stay clear of the substrings other tests count kernels by
    clash = (r"actor_ws_kernel|crowd_actor_kernel|actor_kernel|eval_kernel|eval_ws_kernel|crowd_kernel|crowd_push_kernel|crowd_rvo_kernel|"
             r"policy_ws\w*kernel")
    assert not any(re.search(clash, name) for name, _ in found), found
