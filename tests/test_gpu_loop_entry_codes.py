"""GPU tests of the ORDER of the refusals of the eleven step-loop entry points (`cavoid_actor_run`, `_run_mix`, `_run_ws`,
`cavoid_crowd_actor_run`, `_run_mix`, `_run_ws`, `cavoid_eval_run`, `_run_ws`, `cavoid_crowd_eval_run`, `_run_ws`, `_run_mix`): each is
called raw at the C ABI with inputs that break TWO checks that follow one another in its list and answer with different codes, and must
answer with the code of the earlier one.  The host code around the loop kernels is shared (csrc/cavoid_loop_host.hpp); each entry
point's list of refusals is its own, and its order is what a change to the shared part can silently move.

A 4-agent x 4-world tile env and a 17-agent x 3-world crowd env, both with rows of 7 observed neighbours; loaded `rnn` and weight_sharing
(WS-8) policies of 7 neighbours (the envs') and of 3 (not the envs'); one created-but-unloaded handle of each kind; a holonomic env of each
kind.  No case launches a loop kernel, except the one valid one-step call per entry point that shows the inputs of the other cases are one
or two faults away from a launch.  The expected codes are those of the library before the host code was folded: this file passed
unchanged on that library (loaded through `CAVOID_LIB`) before it was run on the folded one."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = 0, -1, -4
M_ENV, M_OTHER, ACTIONS = 7, 3, 11

# name: (network kind, world kind, signature, the frozen handle: "none" / "optional" / "required")
ENTRY = {
    "cavoid_actor_run": ("rnn", "tile", "actor", "none"),
    "cavoid_actor_run_mix": ("rnn", "tile", "actor", "required"),
    "cavoid_actor_run_ws": ("ws", "tile", "actor", "none"),
    "cavoid_crowd_actor_run": ("rnn", "crowd", "actor", "none"),
    "cavoid_crowd_actor_run_mix": ("rnn", "crowd", "actor", "required"),
    "cavoid_crowd_actor_run_ws": ("ws", "crowd", "actor", "none"),
    "cavoid_eval_run": ("rnn", "tile", "eval", "optional"),
    "cavoid_eval_run_ws": ("ws", "tile", "eval", "optional"),
    "cavoid_crowd_eval_run": ("rnn", "crowd", "eval", "none"),
    "cavoid_crowd_eval_run_ws": ("ws", "crowd", "eval", "optional"),
    "cavoid_crowd_eval_run_mix": ("rnn", "crowd", "eval", "required"),
}
OTHER = {"rnn": "ws", "ws": "rnn", "tile": "crowd", "crowd": "tile"}
WITH_FROZEN = [n for n, v in ENTRY.items() if v[3] != "none"]


def _cfg(n, m):
    from rl_collision_avoidance_amd.config import EnvConfig

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = n
            self.MAX_NUM_OTHER_AGENTS_OBSERVED = m
            EnvConfig.__init__(self)
    return Cfg()


class _World(object):
    """one env with what both signatures need of it: a rollout handle with its buffers, and the evaluation records"""

    def __init__(self, kind, **over):
        from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
        from rl_collision_avoidance_amd.ga3c.evaluate import _EvalRecords
        from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
        w, n = (4, 4) if kind == "tile" else (3, 17)
        self.env = BatchedCollisionAvoidanceEnv(w, _cfg(n, M_ENV), device="cuda:0", seed=5, **over)
        self.roll = BatchedRollout(self.env, None)
        self.roll.reset()
        self.rec = _EvalRecords(self.env)

    def close(self):
        self.roll.close()
        self.env.close()


class _Raw(object):
    """a created-but-unloaded handle (no FusedPolicy is ever unloaded)"""

    def __init__(self, kind):
        from rl_collision_avoidance_amd import _lib
        self._h = C.c_void_p()
        create = _lib.lib().cavoid_policy_create_ws if kind == "ws" else _lib.lib().cavoid_policy_create
        assert create(M_ENV, ACTIONS, 0, C.byref(self._h)) == OK

    def close(self):
        from rl_collision_avoidance_amd import _lib
        _lib.lib().cavoid_policy_destroy(self._h)


@pytest.fixture(scope="module")
def world():
    """every env, policy and handle of the file, made once and left unchanged by the refused calls"""
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    w = {"envs": {}, "pol": {}, "raw": {}}
    for kind in ("tile", "crowd"):
        w["envs"][kind, "actor"] = _World(kind)
        w["envs"][kind, "eval"] = _World(kind, evaluate_mode=1)
        w["envs"][kind, "holonomic"] = _World(kind, dynamics=2)
    for net, arch in (("rnn", "rnn"), ("ws", "weight_sharing")):
        for m in (M_ENV, M_OTHER):
            w["pol"][net, m] = FusedPolicy(NetworkVP_rnn(_cfg(4, m), seed=3, arch=arch).to("cuda:0"), seed=9)
        w["raw"][net] = _Raw(net)
    assert all(p.num_actions == ACTIONS for p in w["pol"].values())
    yield w
    torch.cuda.synchronize()
    for group in ("pol", "raw", "envs"):
        for x in w[group].values():
            x.close()


def _call(name, wd, h, frozen=None, n_steps=1, null_env=False, bad_size=False):
    """the raw call on `wd`'s buffers; frozen is passed where the signature has it"""
    from rl_collision_avoidance_amd import _lib
    _, _, sig, fz = ENTRY[name]
    env, roll, rec = wd.env, wd.roll, wd.rec
    p = lambda t: C.c_void_p(t.data_ptr())
    e = None if null_env else env._h
    handles = (e, h._h) + ((frozen._h if frozen is not None else None,) if fz != "none" else ())
    out = (p(env.rewards), p(env.done), p(env.game_over))
    if sig == "actor":
        b = _lib.CavoidRolloutBuffers.from_buffer_copy(roll._actor_buffers())
        b.struct_size += 8 if bad_size else 0
        args = handles + (roll._h, C.byref(b), p(roll._obs_buffers[0]), p(roll._obs_buffers[1])) + out + (p(roll._act_out), p(roll._val_out))
    else:
        b = _lib.CavoidEvalBuffers.from_buffer_copy(rec.c)
        b.struct_size += 8 if bad_size else 0
        args = handles + (C.byref(b), p(env.obs)) + out + (p(rec.actions), p(rec.values))
    return getattr(_lib.lib(), name)(*args, n_steps, 1, env._stream())


def _wd(world, name, holonomic=False, other_world=False):
    net, kind, sig, _ = ENTRY[name]
    return world["envs"][OTHER[kind] if other_world else kind, "holonomic" if holonomic else sig]


def _good(world, name):
    """the loaded handles of the entry point's kind and the envs' neighbour count: (policy, frozen or None)"""
    net, _, _, fz = ENTRY[name]
    return world["pol"][net, M_ENV], (world["pol"][net, M_ENV] if fz != "none" else None)


@pytest.mark.parametrize("name", list(ENTRY))
def test_the_valid_one_step_call_launches(world, name):
    """the control: what the other cases pass is a launch but for the faults they name"""
    wd = _wd(world, name)
    pol, frozen = _good(world, name)
    assert _call(name, wd, pol, frozen) == OK
    torch.cuda.synchronize()
    if ENTRY[name][3] == "optional":                         # ... and without the frozen handle, where it may be left out
        assert _call(name, wd, pol, None) == OK
        torch.cuda.synchronize()


@pytest.mark.parametrize("name", list(ENTRY))
def test_a_handle_of_the_other_kind_is_refused_before_zero_steps_are_granted(world, name):
    """kind (CAVOID_EUNSUPPORTED) stands before n_steps == 0 (CAVOID_OK)"""
    wrong = world["pol"][OTHER[ENTRY[name][0]], M_ENV]
    assert _call(name, _wd(world, name), wrong, _good(world, name)[1], n_steps=0) == EUNSUPPORTED


@pytest.mark.parametrize("name", list(ENTRY))
def test_zero_steps_are_granted_before_the_handle_is_found_unloaded(world, name):
    """n_steps == 0 (CAVOID_OK) stands before loaded (CAVOID_EINVAL)"""
    unloaded = world["raw"][ENTRY[name][0]]
    assert _call(name, _wd(world, name), unloaded, _good(world, name)[1], n_steps=0) == OK


@pytest.mark.parametrize("name", list(ENTRY))
def test_an_unloaded_handle_is_refused_before_velocity_actions(world, name):
    """loaded (CAVOID_EINVAL) stands before holonomic dynamics (CAVOID_EUNSUPPORTED)"""
    unloaded = world["raw"][ENTRY[name][0]]
    assert _call(name, _wd(world, name, holonomic=True), unloaded, _good(world, name)[1]) == EINVAL


@pytest.mark.parametrize("name", list(ENTRY))
def test_another_neighbour_count_is_refused_before_velocity_actions(world, name):
    """the handles describe one batch (CAVOID_EINVAL) stands before holonomic dynamics (CAVOID_EUNSUPPORTED) -- except in the two crowd
    launches with a required frozen network, which answer a neighbour count that is not the env's with CAVOID_EUNSUPPORTED themselves"""
    narrow = world["pol"][ENTRY[name][0], M_OTHER]
    want = EUNSUPPORTED if name in ("cavoid_crowd_actor_run_mix", "cavoid_crowd_eval_run_mix") else EINVAL
    assert _call(name, _wd(world, name, holonomic=True), narrow, _good(world, name)[1]) == want


# an env of the other kind (CAVOID_EUNSUPPORTED) AND an unloaded frozen handle (CAVOID_EINVAL): which one the entry point meets first
OTHER_WORLD_FIRST = {"cavoid_actor_run_mix": EUNSUPPORTED, "cavoid_eval_run": EUNSUPPORTED, "cavoid_eval_run_ws": EUNSUPPORTED,
                     "cavoid_crowd_eval_run_ws": EUNSUPPORTED,
                     # both handles' loaded flags are read together, before anything about the env
                     "cavoid_crowd_actor_run_mix": EINVAL, "cavoid_crowd_eval_run_mix": EINVAL}


@pytest.mark.parametrize("name", WITH_FROZEN)
def test_the_other_kind_of_world_with_an_unloaded_frozen_handle(world, name):
    assert set(OTHER_WORLD_FIRST) == set(WITH_FROZEN)
    unloaded = world["raw"][ENTRY[name][0]]
    assert _call(name, _wd(world, name, other_world=True), _good(world, name)[0], unloaded) == OTHER_WORLD_FIRST[name]


@pytest.mark.parametrize("name", WITH_FROZEN)
def test_a_frozen_handle_of_the_other_kind_is_refused_before_it_is_found_unloaded(world, name):
    """the frozen handle's kind (CAVOID_EUNSUPPORTED) stands before its loaded flag (CAVOID_EINVAL)"""
    unloaded_other = world["raw"][OTHER[ENTRY[name][0]]]
    assert _call(name, _wd(world, name), _good(world, name)[0], unloaded_other) == EUNSUPPORTED


@pytest.mark.parametrize("name", list(ENTRY))
def test_a_null_env_with_a_bad_struct_size_is_an_argument_error(world, name):
    """both are CAVOID_EINVAL, and neither is looked into: nothing of the env is read before the pointers are checked"""
    pol, frozen = _good(world, name)
    assert _call(name, _wd(world, name), pol, frozen, null_env=True, bad_size=True) == EINVAL
    assert _call(name, _wd(world, name), pol, frozen, null_env=True) == EINVAL
    assert _call(name, _wd(world, name), pol, frozen, bad_size=True) == EINVAL


def test_the_refused_calls_wrote_nothing(world):
    """after every case above: the world buffers of the envs no valid call ran on are as reset left them, and no record moved"""
    torch.cuda.synchronize()
    for kind in ("tile", "crowd"):
        wd = world["envs"][kind, "holonomic"]
        assert int(wd.rec.world_steps.max()) == 0 and wd.roll.step_index == 0
        assert int(wd.roll.emit_t.max()) == -1
