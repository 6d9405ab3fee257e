"""The twin tests of the fused evaluation loops: whole EVALUATE_MODE rounds in launches of K env steps against the same rounds driven step
by step from the host.

tests/test_gpu_eval_fused.py, test_gpu_eval_ws_fused.py, test_gpu_crowd_eval.py, test_gpu_crowd_ws_eval.py and
test_gpu_crowd_eval_mix.py keep their tables and what is truly theirs; the biased networks, the step log, the comparison of two results,
the one cache of step-by-step rounds, the crowd files' reference / fused / same-round triple, the raw C-ABI call and the CLI runner are
here, once.  A plain module: pytest does not rewrite its asserts, so every assert carries a message that names the case and the field."""
import ctypes as C
import os
import subprocess
import sys

import torch

from tests.gpu_support import ROOT

MAX_STEPS = 400
BIAS = 1.0                       # on the favoured logit (the initial weights' logits spread over a few tenths)
NETS = {"straight": 2, "turn": 8, "free": None}
SPLS = (1, 7, 16)                # 7 divides no episode length in particular: launches begin on part-finished tiles
# the tile files' scripted mix: static / non-cooperative / ORCA agents (with gen_frozen_fraction beside it: frozen-network agents too)
MIX = dict(gen_min_agents=2, gen_nonlearning_fraction=0.5, rvo_enabled=1, gen_rvo_fraction=0.34, gen_static_fraction=0.33)


def policy(cfg, net, seed=1234, policy_seed=77, arch="rnn", ws_crowd=False):
    """a FusedPolicy on `NetworkVP_rnn(cfg, arch)` with its random initial weights and BIAS on the logit NETS[net] names, so that the
    argmax depends on the observation but favours one behaviour: "straight" (full speed ahead: goals and collisions), "turn" (turning on
    the spot: time-outs), "free" (none).  `ws_crowd`: the ring handle; None takes the whole-row handle up to 19 observed neighbours and
    the ring handle above."""
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import MAX_OTHERS_WS, FusedPolicy
    model = NetworkVP_rnn(cfg, seed=seed, arch=arch).to("cuda:0")
    if NETS[net] is not None:
        with torch.no_grad():
            model.p_bias[NETS[net]] += BIAS
    if ws_crowd is None:
        ws_crowd = arch == "weight_sharing" and model.max_others > MAX_OTHERS_WS
    return FusedPolicy(model, seed=policy_seed, ws_crowd=ws_crowd)


def close(env, pol, fz=None):
    pol.close()
    if fz is not None:
        fz.close()
    env.close()


class _StepLog(object):
    """wraps env.step of the step-by-step twin: every step's rewards and game_over flags, as the loop saw them"""

    def __init__(self, env):
        self.rew, self.over, self._step = [], [], env.step
        env.step = self

    def __call__(self, actions):
        out = self._step(actions)
        self.rew.append(out[1].clone().view(-1)); self.over.append(out[3].clone())
        return out

    def masked_return(self, N):
        """(the return as include/cavoid.h defines it, restated on the host: the float64 sum, in step order, of the rewards of the steps
        before which the agent's world was not over; which agents the loop paid something AFTER their world was over)"""
        want = torch.zeros_like(self.rew[0], dtype=torch.float64)
        paid_after = torch.zeros_like(self.rew[0], dtype=torch.bool)
        running = torch.ones_like(self.over[0], dtype=torch.bool)
        for rew, over_t in zip(self.rew, self.over):
            live = running.repeat_interleave(N)
            want += torch.where(live, rew.double(), torch.zeros_like(want))
            paid_after |= ~live & (rew != 0)
            running &= over_t == 0
        return want, paid_after

    def world_steps(self):
        """the step at which each world was over (the step count of the round where it never was)"""
        over = torch.stack(self.over).bool()                                   # [T, W]
        first = torch.where(over.any(0), over.int().argmax(0) + 1, torch.full_like(over[0], len(self.over), dtype=torch.int64))
        return first.to(torch.int32)


def _assert_same(ref, ref_state, got, got_state, what, log=None, skip=()):
    """Everything bit for bit.  The return (``per_agent["ret"]``, ``mean_reward``) is held to the step-by-step run twice: bitwise to the
    loop's own sum for every agent the loop paid nothing after its world was over -- and, with ``log``, bitwise to the definition of
    include/cavoid.h (the rewards up to and including the step at which the world is over) for EVERY agent.  The two differ where
    cavoid_step goes on paying a finished world: at the default rewards that is the getting-close penalty of an agent that ran out of
    time within 0.2 m of another (measured: 10 x 48 box scenarios, unbiased network: loop mean_reward -0.19782, kernel -0.13149; the
    4 x 64 scripted mixes likewise), with reward_time_step every agent (test_return_stops_where_the_world_is_over)."""
    masked, paid_after = (None, None)
    if log is not None:
        masked, paid_after = log.masked_return(ref_state[2].numel() // log.over[0].numel())
        if bool(paid_after.any()):
            print("%s: the loop paid %d agent(s) after their world was over; mean_reward loop %.17g kernel %.17g"
                  % (what, int(paid_after.sum()), ref["mean_reward"], got["mean_reward"]))
            skip = tuple(skip) + ("mean_reward", "ret")
    for k in ref:
        if k == "per_agent" or k in skip:
            continue
        assert type(ref[k]) is type(got[k]) and ref[k] == got[k], (what, k, ref[k], got[k])
    assert list(ref) == list(got), (what, "keys", list(ref), list(got))
    for k, t in ref["per_agent"].items():
        if k in skip:
            continue
        assert t.dtype == got["per_agent"][k].dtype and torch.equal(t, got["per_agent"][k]), (what, "per_agent", k)
    if masked is not None:
        learning = ref["per_agent"]["learning"]
        assert torch.equal(got["per_agent"]["ret"], masked), (what, "ret against its definition")
        assert got["mean_reward"] == float(masked[learning].sum()) / max(int(learning.sum()), 1), (what, "mean_reward")
        assert torch.equal(got["per_agent"]["ret"][~paid_after], ref["per_agent"]["ret"][~paid_after]), (what, "ret against the loop's")
    for name, a, b in zip(("f64", "f32", "flags"), ref_state, got_state):
        assert torch.equal(a, b), (what, "final state", name)


def _outcomes(res):
    per = res["per_agent"]
    return set(per["outcome"][per["learning"]].tolist())


def _not_over(env):
    """worlds not over, from the world buffer: cavoid_step's game_over predicate in EVALUATE_MODE"""
    from rl_collision_avoidance_amd import _lib
    fl = env.get_state()[2].view(env.num_worlds, env.max_agents)
    return (((fl & _lib.F_PRESENT) != 0) & ((fl & _lib.F_DONE_MASK) == 0)).any(1)


# ---- the step-by-step rounds: computed once per process ------------------------------------------------------------------------------
_REFS = {}                       # (family, key) -> the round; the family is the test file's, so no two files can collide


def cached(family, key, compute):
    if (family, key) not in _REFS:
        _REFS[(family, key)] = compute()
    return _REFS[(family, key)]


def report_cache(family):
    """the line the last test of an evaluation file ends with: how many step-by-step rounds the file's family holds.  Every cached round
    is computed once per process, so the count is the number of distinct references the file's tables name."""
    n = sum(1 for fam, _ in _REFS if fam == family)
    print("eval twins: %d step-by-step reference round(s) cached for %s (%d in the process)" % (n, family, len(_REFS)))
    return n


def settle_spy(ev, seen):
    """wraps evaluate._settle_finished: the observation buffer as the LAST LAUNCH left it (before evaluate() settles the env), the
    records and the step count; returns the function that puts the original back"""
    settle = ev._settle_finished

    def spy(env_, world_steps, env_steps):
        seen["obs"], seen["world_steps"], seen["env_steps"] = env_.obs.clone(), world_steps.clone(), env_steps
        return settle(env_, world_steps, env_steps)
    ev._settle_finished = spy

    def restore():
        ev._settle_finished = settle
    return restore


class CrowdRounds(object):
    """The crowd files' reference / fused / same-round triple.  `cases`: the file's table, name -> (N, W, ...); `make(name)`: the file's
    (env, policy, frozen policy or None); `switch`: evaluate()'s keyword of the form; `reason`: the name of its unavailable-reason
    function; `run`: the name of evaluate's launch function (the spy of the cut round); `rows_spy(env, name)`: None, or what the file
    notes per step from the step-by-step side's env.policy_rows calls -- it returns (the wrapper, the record kept with the round);
    `also(ev, env, pol, fz)`: what else a file asserts before the fused round."""

    def __init__(self, family, cases, make, switch, reason, run, rows_spy=None, also=None):
        self.family, self.cases, self.make, self.switch, self.reason, self.run = family, cases, make, switch, reason, run
        self.rows_spy, self.also = rows_spy, also

    def reference(self, name, greedy=True, max_steps=MAX_STEPS):
        """evaluate(details=True) of one case, step by step: result, final world buffer, the step log, env.obs at the end, the rows
        record -- computed once"""
        from rl_collision_avoidance_amd.ga3c.evaluate import evaluate

        def compute():
            env, pol, fz = self.make(name)
            log = _StepLog(env)
            record = None
            if self.rows_spy is not None:
                env.policy_rows, record = self.rows_spy(env, name)
            res = evaluate(env, pol, rounds=1, greedy=greedy, max_steps=max_steps, frozen_policy=fz, details=True)
            out = (res, [t.clone() for t in env.get_state()], log, env.obs.clone(), record)
            close(env, pol, fz)
            return out
        return cached(self.family, (name, greedy, max_steps), compute)

    def fused(self, name, spl, greedy=True, max_steps=MAX_STEPS):
        """the same round on the kernel; with it what settle_spy saw"""
        from rl_collision_avoidance_amd.ga3c import evaluate as ev
        env, pol, fz = self.make(name)
        why = getattr(ev, self.reason)(env, pol, fz)
        assert why is None, (name, self.reason, why)           # (no case passes by falling back: the call would raise, too)
        if self.also is not None:
            self.also(ev, env, pol, fz)
        seen = {}
        restore = settle_spy(ev, seen)
        try:
            res = ev.evaluate(env, pol, rounds=1, greedy=greedy, max_steps=max_steps, frozen_policy=fz, steps_per_launch=spl, details=True,
                              **{self.switch: True})
        finally:
            restore()
        state = [t.clone() for t in env.get_state()]
        close(env, pol, fz)
        return res, state, seen

    def same_round(self, name, spl, greedy=True, max_steps=MAX_STEPS):
        N, W = self.cases[name][0], self.cases[name][1]
        ref, ref_state, log, ref_obs, _ = self.reference(name, greedy, max_steps)
        got, got_state, seen = self.fused(name, spl, greedy, max_steps)
        _assert_same(ref, ref_state, got, got_state, (name, spl, greedy), log)
        # the records: the step at which each world was over
        ws = log.world_steps().to(seen["world_steps"].device)
        assert torch.equal(seen["world_steps"], ws), (name, spl, "world_steps")
        assert seen["env_steps"] == ref["env_steps"], (name, spl, "env_steps", seen["env_steps"], ref["env_steps"])
        # the observation of the worlds that ended at the round's last step (or were cut there): the loop stepped them last at that step too
        last = (ws == ref["env_steps"]).nonzero().flatten()
        assert last.numel() >= 1, (name, spl, "no world ended at the round's last step")
        assert torch.equal(seen["obs"].view(W, N, -1)[last], ref_obs.view(W, N, -1)[last]), (name, spl, "obs of the worlds that ended last")

    def cut_at_max_steps(self, name):
        """max_steps = 10 with launches of 7: the last launch is cut to 3, and the round equals the step-by-step round cut at 10"""
        from rl_collision_avoidance_amd.ga3c import evaluate as ev
        launches = []
        run = getattr(ev, self.run)

        def spy(env, policy, frozen_policy, rec, n_steps, greedy=True):
            launches.append(n_steps)
            run(env, policy, frozen_policy, rec, n_steps, greedy)
        setattr(ev, self.run, spy)
        try:
            self.same_round(name, 7, max_steps=10)
        finally:
            setattr(ev, self.run, run)
        assert launches == [7, 3], (name, "launches", launches)
        steps = self.reference(name, max_steps=10)[0]["env_steps"]
        assert steps == 10, (name, "the cut step-by-step round took", steps)


# ---- the C ABI and the CLI ---------------------------------------------------------------------------------------------------------
NO_FROZEN_ARGUMENT = ("cavoid_crowd_eval_run",)              # the entry points without a frozen handle after the learner's


def raw(symbol, env, pol, rec, n, frozen=None, greedy=1, buffers=None, obs=None):
    """straight at the C ABI: the code `symbol` returns"""
    from rl_collision_avoidance_amd import _lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    handles = (env._h, pol._h if pol is not None else None)
    if symbol not in NO_FROZEN_ARGUMENT:
        handles += (frozen._h if frozen is not None else None,)
    return getattr(_lib.lib(), symbol)(*handles, C.byref(buffers if buffers is not None else rec.c), p(env.obs if obs is None else obs),
                                       p(env.rewards), p(env.done), p(env.game_over), p(rec.actions), p(rec.values), n, greedy, env._stream())


def cli(args):
    """ga3c.train --evaluate 1 in a child process; its output"""
    cmd = [sys.executable, "-m", "rl_collision_avoidance_amd.ga3c.train"] + args + ["--evaluate", "1"]
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    run = subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-3000:])
    assert run.returncode == 0, ("ga3c.train", args, "ended with", run.returncode)
    return run.stdout


def last_evaluate_line(out):
    return [l for l in out.splitlines() if l.startswith("[Evaluate] agents ")]


def without_mean_reward(line):
    """mean_reward is the one figure the two definitions of the return may tell apart (include/cavoid.h): left out of the comparison"""
    return " ".join(w for w in line.replace("mean_reward ", "mean_reward=").split("  ") if not w.startswith("mean_reward="))
