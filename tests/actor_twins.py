"""The twin tests of the fused actor loops: one launch of K closed-loop steps against the same K steps taken one launch at a time.

tests/test_gpu_actor.py, test_gpu_actor_ws.py, test_gpu_crowd_actor.py, test_gpu_crowd_ws_actor.py and test_gpu_crowd_actor_mix.py keep
their tables and what is truly theirs; the twin construction, the comparisons, the equality body, the graph-replay and refusal
skeletons, the raw C-ABI call and the train CLI runner are here, once.  A launch form is one row of the table below.  Where the files
differed, the difference is an argument at the call site.  A plain module: pytest does not rewrite its asserts, so every assert
carries a message that names the case, the field and the step."""
import collections
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import torch

from tests import rollout_scripts as rs
from tests.gpu_support import ROOT, _env

# the BatchedRollout methods, the C symbol (and whether a frozen handle follows the learner's) and the availability switches of a form
Form = collections.namedtuple("Form", "run capture symbol frozen_handle available reason")
TILE = Form("run_fused", "capture_fused", "cavoid_actor_run", False, "fused_available", "fused_unavailable_reason")
TILE_WS = Form("run_fused_ws", "capture_fused_ws", "cavoid_actor_run_ws", False, "ws_fused_available", "ws_fused_unavailable_reason")
CROWD = Form("run_fused_crowd", "capture_fused_crowd", "cavoid_crowd_actor_run", False, "crowd_fused_available", "crowd_fused_unavailable_reason")
CROWD_WS = Form("run_fused_crowd_ws", "capture_fused_crowd_ws", "cavoid_crowd_actor_run_ws", False, "crowd_ws_fused_available",
                "crowd_ws_fused_unavailable_reason")
CROWD_MIX = Form("run_fused_crowd_mix", "capture_fused_crowd_mix", "cavoid_crowd_actor_run_mix", True, "crowd_mix_fused_available",
                 "crowd_mix_fused_unavailable_reason")

KS_TILE = (2, 1, 7, 16, 4) + (16,) * 14 + (3,)              # odd counts too: the observation buffers alternate
KS = (2, 1, 7, 16, 4) + (16,) * 7 + (3,)                    # 145 steps; odd counts too: the observation buffers alternate
FAST = dict(max_time_ratio=0.1)
ORCA = dict(rvo_enabled=2, gen_rvo_fraction=0.5, gen_nonlearning_fraction=0.5)

ENV_FIELDS = ("episode", "rewards", "done", "game_over")
RINGS = ("x", "val", "ret", "act_ring", "emit_t")            # the experience rings every form compares
RINGS_DUP = RINGS + ("dup_count",)                          # ... and the re-flush quirk's duplicate counters
STATE = ("state f64", "state f32", "state flags")
INTERLEAVE_ALL = ("obs", "state") + RINGS                   # what the crowd forms compare after the two forms took turns
INTERLEAVE_TILE = ("obs", "emit_t")                         # ... and the tile forms
DRAINED = ("src", "x", "r", "a_index")


def make(W, N, M, seed, reflush=False, greedy=False, arch="rnn", net_M=None, ws_crowd=None, frozen=False, skip_finished=None,
         dup_capacity=600000, time_max=5, **over):
    """(env, net, policy, rollout) of one twin.  `net_M`: a network made for another neighbour count than the env's.  `ws_crowd`: the ring
    handle; None takes the whole-row handle up to 19 observed neighbours and the ring handle above.  `frozen`: False, "rnn" (a second
    network of its own weights), "learner" (the learner's handle serves) or "from_fraction" ("rnn" where the generator makes
    frozen-network agents).  `skip_finished`: None is `not reflush` -- the fused kernels hand a result only to the rows that still need an
    action (with the re-flush quirk: to every row), exactly the rows the step-by-step path lists with skip_finished, so like is compared
    with like.  `dup_capacity`: room for every duplicate row of the re-flush quirk (a full buffer drops rows in arrival order, which
    legitimately differs between the two forms)."""
    from rl_collision_avoidance_amd.config import EnvConfig
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import MAX_OTHERS_WS, FusedPolicy
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    env = _env(W, N, M, seed=seed, **over)
    cfg = env.config
    if net_M is not None:

        class Cfg(EnvConfig):
            def __init__(self):
                self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
                self.MAX_NUM_OTHER_AGENTS_OBSERVED = net_M
                EnvConfig.__init__(self)
        cfg = Cfg()
    torch.manual_seed(1234)
    net = NetworkVP_rnn(cfg, arch=arch).to("cuda:0")
    if ws_crowd is None:
        ws_crowd = arch == "weight_sharing" and net.max_others > MAX_OTHERS_WS
    pol = FusedPolicy(net, seed=77, ws_crowd=ws_crowd)
    if frozen == "from_fraction":
        frozen = "rnn" if over.get("gen_frozen_fraction", 0.0) > 0.0 else False
    fz = None
    if frozen == "rnn":                                      # the network behind the frozen-network agents: its own weights
        torch.manual_seed(4321)
        fz = FusedPolicy(NetworkVP_rnn(cfg).to("cuda:0"), seed=0)
    elif frozen == "learner":
        fz = pol
    else:
        assert frozen is False, ("make: frozen", frozen)
    roll = BatchedRollout(env, pol, reflush_done=reflush, greedy=greedy, time_max=time_max, dup_capacity=dup_capacity if reflush else None,
                          skip_finished=(not reflush) if skip_finished is None else skip_finished, frozen_policy=fz)
    roll.reset()
    return env, net, pol, roll


def same(a, b, what):
    assert torch.equal(a, b), what


def close(*pairs):
    for env, roll in pairs:
        roll.close(); env.close()


def compare_twins(env_a, a, env_b, b, total, rings=RINGS_DUP, case=None):
    """observation, world state, the env's outputs, the experience rings and the step counter, bit for bit"""
    same(a.obs, b.obs, (case, "obs", total))
    for name, x, y in zip(STATE, env_a.get_state(), env_b.get_state()):
        same(x, y, (case, name, total))
    for name in ENV_FIELDS:
        same(getattr(env_a, name), getattr(env_b, name), (case, name, total))
    for name in rings:
        same(getattr(a, name), getattr(b, name), (case, name, total))
    assert a.step_index == b.step_index == total, (case, "step_index", a.step_index, b.step_index, total)


def compare_interleaved(env_a, a, env_b, b, fields=INTERLEAVE_ALL, case=None):
    """after the two forms took turns on both twins: each continues where the other stopped"""
    for name in fields:
        if name == "state":
            for sname, x, y in zip(STATE, env_a.get_state(), env_b.get_state()):
                same(x, y, (case, "interleaved", sname))
        else:
            same(getattr(a, name), getattr(b, name), (case, "interleaved", name))


def compare_drained(ba, bb, case=None):
    """what reaches the trainer: the rows in the order of their provenance"""
    ka = np.lexsort(ba.src.cpu().numpy().T[::-1])
    kb = np.lexsort(bb.src.cpu().numpy().T[::-1])
    for name in DRAINED:
        assert np.array_equal(getattr(ba, name).cpu().numpy()[ka], getattr(bb, name).cpu().numpy()[kb]), (case, "drained", name)


def compare_episode_records(ea, eb, case=None):
    """what reaches the stats process: counters exact, the totals to float32 rounding (double atomics whose order varies)"""
    ea, eb = ea[np.lexsort(ea.T[::-1])], eb[np.lexsort(eb.T[::-1])]
    for col in (0, 2):
        assert np.array_equal(ea[:, col], eb[:, col]), (case, "episode records", "column %d" % col)
    np.testing.assert_allclose(ea[:, 1], eb[:, 1], rtol=1e-6, atol=1e-6, err_msg=str((case, "episode records", "column 1")))


def step_side(label, N, W, M, reflush, extra=None):
    """The crowd files' conditions on the step-by-step side (the code of before): it did what the case is about, so that nothing passes on
    nothing -- and the line GPU logs are read by.  `extra(total)` returns the words a file adds to the line."""
    def check(env_b, b, bb, eb, dup_b, total):
        more = extra(total) if extra is not None else ""
        print("%s N=%d W=%d M=%d: step-by-step side: %sepisode max %d, drained %d rows, %d duplicates (%d dropped), %d episode records"
              % (label, N, W, M, more, env_b.episode.max().item(), len(bb), dup_b[0], dup_b[1], len(eb)))
        assert env_b.episode.max().item() >= 1, (label, "no episode ended on the step-by-step side")
        assert len(bb) > 0 and len(eb) > 0, (label, "step-by-step side: rows drained, episode records", len(bb), len(eb))
        assert dup_b[1] == 0 and (dup_b[0] > 0 if reflush else dup_b[0] == 0), (label, "dup_count on the step-by-step side", dup_b, reflush)
    return check


def fused_equals_step_by_step(form, twin_a, twin_b, case, ks=KS, compare_at=None, compare_at_end=False, rings=RINGS_DUP, step_form=None,
                              check_step_side=None, deep_flushes=None, interleave=INTERLEAVE_ALL):
    """The equality body.  `twin_a` runs `form.run(k)` for every k of `ks`, `twin_b` k times step(); after every launch for which
    `compare_at(total)` holds (None: every launch; `compare_at_end`: once more after the last) the twins are compared on `rings`, and
    both envs must report `step_form` (None: not asked).  Then what reaches the trainer and the stats process, and the interleave on
    the `interleave` fields.  `check_step_side` (see step_side): the crowd files' conditions on the step-by-step side; without it the
    fused side's episode counter must have moved.  `deep_flushes`: (time_max, tag) for rollout_scripts.require_deep_flushes.  Closes
    both twins."""
    (env_a, net_a, _, a), (env_b, net_b, _, b) = twin_a, twin_b
    for i, (p, q) in enumerate(zip(net_a.parameters(), net_b.parameters())):
        assert torch.equal(p, q), (case, "the twins' networks differ in parameter", i)
    same(a.obs, b.obs, (case, "first observation"))
    run_a, run_b = getattr(a, form.run), getattr(b, form.run)
    total = 0
    for k in ks:
        run_a(k)
        for _ in range(k):
            b.step()
        total += k
        if compare_at is not None and not compare_at(total):
            continue
        compare_twins(env_a, a, env_b, b, total, rings, case)
        if step_form is not None:
            assert env_a.last_step_form == step_form and env_b.last_step_form == step_form, (
                case, "last_step_form", total, env_a.last_step_form, env_b.last_step_form, step_form)
    if compare_at_end:
        compare_twins(env_a, a, env_b, b, total, rings, case)
    if check_step_side is None:
        assert env_a.episode.max().item() >= 1, (case, "no world restarted: restarts must be inside what was compared")
    dup_b = b.dup_count.tolist()
    ba, bb = a.drain(flush_all=True), b.drain(flush_all=True)
    ea, eb = a.drain_episodes().cpu().numpy(), b.drain_episodes().cpu().numpy()
    if check_step_side is not None:
        check_step_side(env_b, b, bb, eb, dup_b, total)
    if deep_flushes is not None:
        rs.require_deep_flushes(bb.src.cpu().numpy(), *deep_flushes)
    # what reaches the trainer and the stats process
    assert len(ba) == len(bb) > 0, (case, "drained rows", len(ba), len(bb))
    assert ba.dropped == bb.dropped == 0, (case, "dropped rows", ba.dropped, bb.dropped)
    compare_drained(ba, bb, case)
    assert len(ea) == len(eb) > 0, (case, "episode records", len(ea), len(eb))
    compare_episode_records(ea, eb, case)
    # and the two forms interleave: each continues where the other stopped
    a.step(); run_a(3)
    run_b(2); b.step(); b.step()
    compare_interleaved(env_a, a, env_b, b, interleave, case)
    close((env_a, a), (env_b, b))


def graph_replay(form, twin_a, twin_b, replays, compare, eager=True, one_more_step=False, refused_steps_per_graph=None):
    """`form.capture(steps_per_graph=4)` -- which runs 2 warm-up steps outside the capture -- and `replays` replays on `twin_a` against
    the same steps on `twin_b`: eager `form.run` calls (`eager`) or step() calls.  `compare(env_a, a, env_b, b, total)` is the file's
    comparison.  `one_more_step`: one more step() on each side lands in the same ring block and draws the same actions only if the
    rollout's and the policy's device-side step counters agree.  `refused_steps_per_graph`: a count the capture must refuse.  Leaves
    the twins open."""
    (env_a, _, _, a), (env_b, _, _, b) = twin_a, twin_b
    getattr(a, form.capture)(steps_per_graph=4)
    total = 2 + 4 * replays
    if eager:
        getattr(b, form.run)(2)
    a.replay(replays)
    if eager:
        for _ in range(replays):
            getattr(b, form.run)(4)
    else:
        for _ in range(total):
            b.step()
    compare(env_a, a, env_b, b, total)
    if one_more_step:
        a.step(); b.step()
        compare(env_a, a, env_b, b, total + 1)
        assert (a.emit_t >= 0).any(), (form.capture, "no row was emitted")
    if refused_steps_per_graph is not None:
        try:
            getattr(a, form.capture)(steps_per_graph=refused_steps_per_graph)
        except ValueError:
            pass
        else:
            raise AssertionError("%s(steps_per_graph=%d) was not refused" % (form.capture, refused_steps_per_graph))


def raw_run(form, env, roll, pol, n_steps=2, fz=None, cur=None, same_buffer=False):
    """straight at the C ABI: the code `form.symbol` returns.  `cur`: which observation buffer is handed over as the current one (None:
    the rollout's); `same_buffer`: the same buffer as the next one too (an argument error)."""
    from rl_collision_avoidance_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr())
    cur = roll._cur if cur is None else cur
    handles = (env._h, pol._h) + ((fz._h if fz is not None else None,) if form.frozen_handle else ()) + (roll._h,)
    b = roll._actor_buffers()
    rc = getattr(_lib.lib(), form.symbol)(*handles, C.byref(b), p(roll._obs_buffers[cur]), p(roll._obs_buffers[cur if same_buffer else 1 - cur]),
                                          p(env.rewards), p(env.done), p(env.game_over), p(roll._act_out), p(roll._val_out), n_steps, 0, None)
    torch.cuda.synchronize()
    return rc


def refused(form, env, pol, roll, code, word, fz=None, cur=None, reason_in_error=False, error_match=None, state_untouched=False):
    """A rollout the form does not carry: the reason names `word`, the switch says no, `form.run` raises RuntimeError (`reason_in_error`:
    with the reason in it; `error_match`: with these words) and the C entry point returns `code` -- a code, not a crash
    (`state_untouched`: and leaves the world buffer alone)."""
    why = getattr(roll, form.reason)
    assert why is not None and word in why, (form.reason, word, why)
    assert not getattr(roll, form.available), (form.available, "says yes beside the reason", why)
    try:
        getattr(roll, form.run)(2)
    except RuntimeError as err:
        assert not reason_in_error or why in str(err), (form.run, "the error does not carry the reason", str(err), why)
        assert error_match is None or error_match in str(err), (form.run, "the error does not say", error_match, str(err))
    else:
        raise AssertionError("%s(2) ran where %s says: %s" % (form.run, form.reason, why))
    state = [t.clone() for t in env.get_state()]
    rc = raw_run(form, env, roll, pol, fz=fz, cur=cur)
    assert rc == code, (form.symbol, "returned", rc, "expected", code, "for", word)
    if state_untouched:
        for name, u, v in zip(STATE, state, env.get_state()):
            assert torch.equal(u, v), (form.symbol, "refused with", code, "but wrote", name)
    return roll


def unchanged_by(call, tensors, what):
    """`call()` must leave every tensor `tensors()` lists as it was; returns what `call()` returned"""
    before = [t.clone() for t in tensors()]
    out = call()
    for i, (u, v) in enumerate(zip(before, tensors())):
        assert torch.equal(u, v), (what, "changed tensor", i)
    return out


def train_cli(tmp_path, args):
    """ga3c.train in a child process on a 64-world batch, 300 episodes; the end of its output is printed"""
    cmd = [sys.executable, "-m", "rl_collision_avoidance_amd.ga3c.train"] + args + ["--worlds", "64", "--episodes", "300", "--pretrain-steps", "0",
                                                                                      "--print-every", "100", "--train-rows", "2048",
                                                                                      "--checkpoint-dir", str(tmp_path / "ck")]
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    run = subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-3000:])
    return run


def train_cli_runs_the_kernel(tmp_path, args, line):
    run = train_cli(tmp_path, args)
    assert run.returncode == 0, ("ga3c.train", args, "ended with", run.returncode)
    assert line in run.stdout, ("ga3c.train", args, "did not print", line)
    assert "finished" in run.stdout and " 0 training steps" not in run.stdout, ("ga3c.train", args, "did not train to the end")


def train_cli_prints_todays_line(tmp_path, args, line, symbol):
    run = train_cli(tmp_path, args)
    assert run.returncode == 0, ("ga3c.train", args, "ended with", run.returncode)
    assert line in run.stdout, ("ga3c.train", args, "did not print", line)
    assert symbol not in run.stdout and "finished" in run.stdout, ("ga3c.train", args, "named", symbol, "or did not finish")
