"""``evaluate`` -- EVALUATE_MODE runs (Config.EVALUATE_MODE: every agent of a world must finish; actions are the argmax,
/root/reference/ga3c/GA3C/ProcessAgent.py:98-103) with the per-agent outcome statistics the collision-avoidance papers
report: reached the goal / collided / ran out of time, and the extra time to goal.  Worlds are stepped WITHOUT auto-reset
(``cavoid_step``), so that every agent's terminal flags can be read from the world buffer once its world is over.

Two paths produce the same numbers: the step-by-step loop (policy launch, ``env.step`` and a look at the world buffer per env
step, one host synchronisation each) and, with ``fused=True``, ``cavoid_eval_run`` -- the whole loop per tile of worlds inside
one launch of ``steps_per_launch`` steps that finished tiles leave early, the outcome recorded on the device (``fused_ws=True``:
``cavoid_eval_run_ws``, the same for the ``weight_sharing`` network; ``fused_crowd=True``: ``cavoid_crowd_eval_run``, the same for
crowd worlds of 17 to 64 agents and the ``rnn`` network; ``fused_crowd_ws=True``: ``cavoid_crowd_eval_run_ws``, crowd worlds and the
``weight_sharing`` network; ``fused_crowd_mix=True``: ``cavoid_crowd_eval_run_mix``, crowd worlds, the ``rnn`` network and a second,
frozen ``rnn`` network for the frozen-network agents)."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from .. import _lib
from ..batched_env import BatchedCollisionAvoidanceEnv

# per_agent["outcome"] codes (over ALL agent slots; the rates count the learning ones)
OUTCOME_UNFINISHED, OUTCOME_GOAL, OUTCOME_COLLISION, OUTCOME_TIMEOUT = 0, 1, 2, 3
_MAX_OTHERS_FUSED = 19       # kPolMaxOthers: the kernel parks the whole input row (policy_kernel.MAX_OTHERS)


def _percentile(sorted_vals: torch.Tensor, q: float) -> float:
    """numpy.percentile's default (linear interpolation between the two nearest ranks) of an ascending float64 vector; 0.0 when empty."""
    n = int(sorted_vals.numel())
    if n == 0:
        return 0.0
    pos = q / 100.0 * (n - 1)
    lo = int(pos)
    hi = min(lo + 1, n - 1)
    a, b = float(sorted_vals[lo]), float(sorted_vals[hi])
    return a + (b - a) * (pos - lo)


def reduce_outcomes(rounds: Sequence[dict], dt: float, near_goal_threshold: float, details: bool = False) -> Dict[str, object]:
    """The evaluation result from what the rounds recorded -- a pure function of tensors, the one both paths of ``evaluate`` end in.

    Each round is a dict of
      ``ret`` float64 [A]        the agents' returns,
      ``goal_step`` int [A]      the env step at which the agent first stood at its goal (0: never; such an agent's time is not counted),
      ``env_steps`` int          steps the round took (the step-by-step loop's count = the largest ``world_steps``),
      ``state0`` (f64 [4,A], f32 [5,A], flags [A])   the world buffer right after the reset (``env.get_state()``),
      ``flags_end`` int [A]      the flags when the round was over.
    An agent that stands at its goal counts as goal whatever else its flags say; then collision; then timeout.  Rates are over the
    learning agents that were present.  ``details`` adds the 75th / 90th percentile of the extra time to goal and the ``per_agent``
    tensors (the rounds concatenated): ``outcome`` int8 (OUTCOME_*), ``time_to_goal`` / ``extra_time`` float64 (0 where not counted),
    ``ret`` float64, ``learning`` bool."""
    tot = {"agents": 0, "goal": 0, "collision": 0, "timeout": 0, "reward": 0.0, "steps": 0, "time_to_goal": 0.0, "extra_time": 0.0}
    per: Dict[str, List[torch.Tensor]] = {"outcome": [], "time_to_goal": [], "extra_time": [], "ret": [], "learning": []}
    for r in rounds:
        f64_0, f32_0, fl_0 = r["state0"]
        fl, ret, goal_step = r["flags_end"], r["ret"], r["goal_step"]
        present = (fl_0 & _lib.F_PRESENT) != 0
        learning = present & ((fl_0 & _lib.F_LEARNING) != 0)
        # straight-line time at the preferred speed = the yardstick for "extra time to goal"
        dist = torch.sqrt((f64_0[0] - f32_0[0].double()) ** 2 + (f64_0[1] - f32_0[1].double()) ** 2)
        straight = ((dist - float(near_goal_threshold)).clamp_min(0.0) / f32_0[3].double().clamp_min(1e-6))
        t_goal = goal_step.double() * float(dt)
        at_goal = (fl & _lib.F_AT_GOAL) != 0
        in_coll = ((fl & _lib.F_IN_COLL) != 0) & ~at_goal
        ran_out = ((fl & _lib.F_RAN_OUT) != 0) & ~at_goal & ~in_coll
        goal, coll, tout = learning & at_goal, learning & in_coll, learning & ran_out
        timed = goal & (goal_step > 0)
        tot["agents"] += int(learning.sum()); tot["goal"] += int(goal.sum()); tot["collision"] += int(coll.sum())
        tot["timeout"] += int(tout.sum()); tot["reward"] += float(ret[learning].sum()); tot["steps"] += int(r["env_steps"])
        tot["time_to_goal"] += float(t_goal[timed].sum()); tot["extra_time"] += float((t_goal[timed] - straight[timed]).sum())
        if details:
            outcome = torch.zeros_like(fl, dtype=torch.int8)
            outcome[at_goal] = OUTCOME_GOAL; outcome[in_coll] = OUTCOME_COLLISION; outcome[ran_out] = OUTCOME_TIMEOUT
            counted = at_goal & (goal_step > 0)
            zero = torch.zeros_like(t_goal)
            per["outcome"].append(outcome); per["learning"].append(learning); per["ret"].append(ret.clone())
            per["time_to_goal"].append(torch.where(counted, t_goal, zero)); per["extra_time"].append(torch.where(counted, t_goal - straight, zero))
    n, g = max(tot["agents"], 1), max(tot["goal"], 1)
    res: Dict[str, object] = {
        "agents": tot["agents"], "success_rate": tot["goal"] / n, "collision_rate": tot["collision"] / n,
        "timeout_rate": tot["timeout"] / n, "unfinished_rate": 1.0 - (tot["goal"] + tot["collision"] + tot["timeout"]) / n,
        "mean_reward": tot["reward"] / n, "mean_time_to_goal": tot["time_to_goal"] / g,
        "mean_extra_time_to_goal": tot["extra_time"] / g, "env_steps": tot["steps"]}
    if details:
        per_agent = {k: (torch.cat(v) if v else torch.zeros(0)) for k, v in per.items()}
        sel = per_agent["learning"] & (per_agent["outcome"] == OUTCOME_GOAL) & (per_agent["time_to_goal"] > 0) if rounds else None
        extra = torch.sort(per_agent["extra_time"][sel].double().cpu())[0] if rounds else torch.zeros(0, dtype=torch.float64)
        res["extra_time_p75"], res["extra_time_p90"] = _percentile(extra, 75.0), _percentile(extra, 90.0)
        res["per_agent"] = per_agent
    return res


def evaluate_fused_unavailable_reason(env, policy, frozen_policy=None) -> Optional[str]:
    """Why ``evaluate(fused=True)`` (``cavoid_eval_run``: the evaluation loop inside one launch) does not apply to this env and policy --
    None when it does.  Host values only (no launch, no GPU): what ``cavoid_eval_run`` answers CAVOID_EUNSUPPORTED to, which is what
    ``cavoid_actor_run`` / ``_run_mix`` refuse -- crowd worlds, the weight_sharing network, wide rows, velocity actions, a non-default
    inference form, frozen-network agents without their network -- and a policy that is no ``FusedPolicy`` at all."""
    n = int(env.max_agents)
    if not hasattr(policy, "act") or not hasattr(policy, "inference_form") or getattr(policy, "_h", None) is None:
        return "the policy is not a FusedPolicy (a plain callable is evaluated step by step)"
    if n > _lib.TILE_MAX_AGENTS:
        return "%d agents per world: crowd worlds (more than %d) are evaluated step by step" % (n, _lib.TILE_MAX_AGENTS)
    for who, pol in (("policy", policy), ("frozen policy", frozen_policy)):
        if pol is None:
            continue
        if getattr(pol, "ws", False) or getattr(pol, "arch", "rnn") != "rnn":
            return "the %s is the %s network (the evaluation kernel embeds the LSTM pass)" % (who, getattr(pol, "arch", "weight_sharing"))
        if int(pol.max_others) > _MAX_OTHERS_FUSED:
            return "the %s observes %d neighbours (the evaluation kernel parks the whole row: up to %d)" % (who, int(pol.max_others), _MAX_OTHERS_FUSED)
        if tuple(pol.inference_form) != ("split", 16):
            return "the %s runs a non-default inference form %r (CAVOID_POLICY_F32 / CAVOID_POLICY_PRODUCTS at its creation)" % (
                who, tuple(pol.inference_form))
    if int(policy.max_others) != int(env.max_other):
        return "the policy observes %d neighbours, the env's rows carry %d" % (int(policy.max_others), int(env.max_other))
    if frozen_policy is not None and int(frozen_policy.max_others) != int(policy.max_others):
        return "the frozen policy observes %d neighbours, the policy %d" % (int(frozen_policy.max_others), int(policy.max_others))
    if int(env.cfg.dynamics) == 2:
        return "holonomic (velocity) actions"
    if frozen_policy is None and float(env.cfg.gen_frozen_fraction) > 0.0 and float(env.cfg.gen_nonlearning_fraction) > 0.0:
        return "frozen-network agents without a frozen_policy (they act by their own network)"
    from .rollout import env_step_lds_bytes
    lent = 2 * 64 * 528          # 2 * kSpPlaneB: the two activation planes the policy pass lends the env step
    need = env_step_lds_bytes(n, 6 + 7 * int(env.max_other), bool(env.cfg.rvo_enabled))
    if bool(env.cfg.rvo_enabled) and need > lent:
        return "the env step's LDS with the ORCA lines (%d bytes) does not fit the %d bytes the policy pass lends it" % (need, lent)
    return None


def evaluate_fused_ws_unavailable_reason(env, policy, frozen_policy=None) -> Optional[str]:
    """Why ``evaluate(fused_ws=True)`` (``cavoid_eval_run_ws``: the evaluation loop of the weight_sharing network inside one launch) does
    not apply to this env and policy -- None when it does.  Host values only (no launch, no GPU), the refusals of the C entry point one
    for one: a ``FusedPolicy`` of the ``weight_sharing`` network on the whole-row kernels (up to ``MAX_OTHERS_WS`` observed neighbours, not
    the ring handle of ``ws_crowd=True``) whose neighbour count is the env's, tile worlds (up to 16 agents), table actions, a frozen
    policy of the same kind for the frozen-network agents, and an env step whose LDS fits the rows the pass lends it."""
    from .policy_kernel import MAX_OTHERS_WS
    from .rollout import WS_ACTOR_LENT_BYTES, env_step_lds_bytes
    n = int(env.max_agents)
    if not hasattr(policy, "act") or not hasattr(policy, "inference_form") or getattr(policy, "_h", None) is None:
        return "the policy is not a FusedPolicy (a plain callable is evaluated step by step)"
    if not getattr(policy, "ws", False):
        return "the policy is the %s network (use fused=True: cavoid_eval_run embeds the LSTM pass)" % (getattr(policy, "arch", "rnn"),)
    if getattr(policy, "crowd", False) or int(policy.max_others) > MAX_OTHERS_WS:
        return ("the policy observes %d neighbours on the ring kernels (the weight_sharing evaluation kernel parks the whole row: up to %d; "
                "the ring form is evaluated step by step)" % (int(policy.max_others), MAX_OTHERS_WS))
    if int(policy.max_others) != int(env.max_other):
        return "the policy observes %d neighbours, the env's rows carry %d" % (int(policy.max_others), int(env.max_other))
    if n > _lib.TILE_MAX_AGENTS:
        return "%d agents per world: crowd worlds (more than %d) are evaluated step by step" % (n, _lib.TILE_MAX_AGENTS)
    if int(env.cfg.dynamics) == 2:
        return "holonomic (velocity) actions"
    if frozen_policy is not None:
        fz = frozen_policy
        same_kind = getattr(fz, "_h", None) is not None and getattr(fz, "ws", False) and not getattr(fz, "crowd", False)
        if not same_kind or int(fz.max_others) != int(policy.max_others) or int(getattr(fz, "num_actions", 0)) != int(getattr(policy, "num_actions", 0)):
            return ("the frozen policy is not a weight_sharing FusedPolicy of the policy's shape (%s, %d neighbours; the policy: %d)"
                    % (getattr(fz, "arch", "no FusedPolicy"), int(getattr(fz, "max_others", -1)), int(policy.max_others)))
    elif float(env.cfg.gen_frozen_fraction) > 0.0 and float(env.cfg.gen_nonlearning_fraction) > 0.0:
        return "frozen-network agents without a frozen_policy (they act by their own network)"
    need = env_step_lds_bytes(n, 6 + 7 * int(env.max_other), bool(env.cfg.rvo_enabled))
    if need > WS_ACTOR_LENT_BYTES:
        return "the env step's LDS (%d bytes) does not fit the %d bytes the weight_sharing pass lends it" % (need, WS_ACTOR_LENT_BYTES)
    return None


def evaluate_fused_crowd_unavailable_reason(env, policy, frozen_policy=None) -> Optional[str]:
    """Why ``evaluate(fused_crowd=True)`` (``cavoid_crowd_eval_run``: the evaluation loop of crowd worlds inside one launch) does not apply
    to this env and policy -- None when it does.  Host values only (no launch, no GPU), the refusals of the C entry point one for one
    (what ``cavoid_crowd_actor_run`` refuses): worlds of 17..64 agents (tile worlds have ``fused=True``), a ``FusedPolicy`` of the ``rnn``
    network on the default inference form whose neighbour count is the env's, table actions, and no frozen-network agents (the launch
    carries one network).  The entry point's last refusal, an env step whose LDS exceeds what the policy pass lends it, has no case here:
    ``cavoid_create`` admits no crowd env whose step takes more than that."""
    n = int(env.max_agents)
    if not hasattr(policy, "act") or not hasattr(policy, "inference_form") or getattr(policy, "_h", None) is None:
        return "the policy is not a FusedPolicy (a plain callable is evaluated step by step)"
    if n <= _lib.TILE_MAX_AGENTS:
        return "%d agents per world: up to %d run the tile forms' evaluation kernel (fused=True / cavoid_eval_run)" % (n, _lib.TILE_MAX_AGENTS)
    if getattr(policy, "ws", False) or getattr(policy, "arch", "rnn") != "rnn":
        return ("the policy is the %s network (the crowd evaluation kernel embeds the LSTM pass; the weight_sharing ring form is evaluated "
                "step by step)" % (getattr(policy, "arch", "weight_sharing"),))
    if int(env.cfg.dynamics) == 2:
        return "holonomic (velocity) actions"
    if tuple(policy.inference_form) != ("split", 16):
        return "the policy runs a non-default inference form %r (CAVOID_POLICY_F32 / CAVOID_POLICY_PRODUCTS at its creation)" % (
            tuple(policy.inference_form),)
    if int(policy.max_others) != int(env.max_other):
        return "the policy observes %d neighbours, the env's rows carry %d" % (int(policy.max_others), int(env.max_other))
    if frozen_policy is not None:
        return "a frozen_policy (the crowd evaluation kernel carries one network: there is no frozen form of this launch)"
    if float(env.cfg.gen_frozen_fraction) > 0.0 and float(env.cfg.gen_nonlearning_fraction) > 0.0:
        return "frozen-network agents (the crowd evaluation kernel carries one network; they act by their own)"
    return None


def evaluate_fused_crowd_ws_unavailable_reason(env, policy, frozen_policy=None) -> Optional[str]:
    """Why ``evaluate(fused_crowd_ws=True)`` (``cavoid_crowd_eval_run_ws``: the evaluation loop of crowd worlds with the weight_sharing
    network inside one launch) does not apply to this env and policy -- None when it does.  Host values only (no launch, no GPU), the
    refusals of the C entry point one for one: a ``FusedPolicy`` of the ``weight_sharing`` network -- on the whole-row handle (up to
    ``MAX_OTHERS_WS`` observed neighbours) or the ring handle (``ws_crowd=True``) alike -- worlds of 17..64 agents (tile worlds have
    ``fused_ws=True``), table actions, a neighbour count that is the env's, a frozen policy that is a weight_sharing ``FusedPolicy`` of
    the policy's shape for the frozen-network agents, and a crowd env step whose LDS fits the rows the pass lends it.  That last refusal
    has no case here: ``cavoid_create`` admits no crowd env whose step takes more than that; the check stands for a library that does."""
    from .rollout import WS_ACTOR_LENT_BYTES, crowd_env_step_lds_bytes
    n = int(env.max_agents)
    if not hasattr(policy, "act") or not hasattr(policy, "inference_form") or getattr(policy, "_h", None) is None:
        return "the policy is not a FusedPolicy (a plain callable is evaluated step by step)"
    if not getattr(policy, "ws", False):
        return ("the policy is the %s network (use fused_crowd=True: cavoid_crowd_eval_run embeds the LSTM pass)" % (getattr(policy, "arch", "rnn"),))
    if n <= _lib.TILE_MAX_AGENTS:
        return ("%d agents per world: up to %d run the tile forms' weight_sharing evaluation kernel (fused_ws=True / cavoid_eval_run_ws)"
                % (n, _lib.TILE_MAX_AGENTS))
    if int(env.cfg.dynamics) == 2:
        return "holonomic (velocity) actions"
    if int(policy.max_others) != int(env.max_other):
        return "the policy observes %d neighbours, the env's rows carry %d" % (int(policy.max_others), int(env.max_other))
    if frozen_policy is not None:
        fz = frozen_policy
        same_kind = getattr(fz, "_h", None) is not None and getattr(fz, "ws", False)
        if not same_kind or int(fz.max_others) != int(policy.max_others) or int(getattr(fz, "num_actions", 0)) != int(getattr(policy, "num_actions", 0)):
            return ("the frozen policy is not a weight_sharing FusedPolicy of the policy's shape (%s, %d neighbours; the policy: %d)"
                    % (getattr(fz, "arch", "no FusedPolicy"), int(getattr(fz, "max_others", -1)), int(policy.max_others)))
    elif float(env.cfg.gen_frozen_fraction) > 0.0 and float(env.cfg.gen_nonlearning_fraction) > 0.0:
        return "frozen-network agents without a frozen_policy (they act by their own network)"
    need = crowd_env_step_lds_bytes(n, 6 + 7 * int(env.max_other))
    if need > min(65536, WS_ACTOR_LENT_BYTES):
        return ("the crowd env step's LDS (%d bytes) does not fit the %d bytes the weight_sharing pass lends it"
                % (need, min(65536, WS_ACTOR_LENT_BYTES)))
    return None


def evaluate_fused_crowd_mix_unavailable_reason(env, policy, frozen_policy=None) -> Optional[str]:
    """Why ``evaluate(fused_crowd_mix=True)`` (``cavoid_crowd_eval_run_mix``: the evaluation loop of crowd worlds with a second, frozen
    network for the frozen-network agents inside one launch) does not apply to this env and the two policies -- None when it does.  Host
    values only (no launch, no GPU), the refusals of the C entry point one for one: what ``evaluate_fused_crowd_unavailable_reason``
    asks of the env and the policy, and a ``frozen_policy`` that is a ``FusedPolicy`` of the ``rnn`` network on the default inference form
    with the policy's neighbour count and action count.  Without a ``frozen_policy`` the launch has nothing to add: ``fused_crowd=True``
    is the one-network form.  The entry point's last refusal, an env step whose LDS exceeds what the policy pass lends it, has no case
    here: ``cavoid_create`` admits no crowd env whose step takes more than that."""
    n = int(env.max_agents)
    if not hasattr(policy, "act") or not hasattr(policy, "inference_form") or getattr(policy, "_h", None) is None:
        return "the policy is not a FusedPolicy (a plain callable is evaluated step by step)"
    if n <= _lib.TILE_MAX_AGENTS:
        return ("%d agents per world: up to %d run the tile forms' evaluation kernel (fused=True / cavoid_eval_run, with its frozen_policy)"
                % (n, _lib.TILE_MAX_AGENTS))
    if getattr(policy, "ws", False) or getattr(policy, "arch", "rnn") != "rnn":
        return ("the policy is the %s network (the crowd mix evaluation kernel embeds the LSTM pass; fused_crowd_ws=True / "
                "cavoid_crowd_eval_run_ws carries weight_sharing and its frozen_policy)" % (getattr(policy, "arch", "weight_sharing"),))
    if int(env.cfg.dynamics) == 2:
        return "holonomic (velocity) actions"
    if tuple(policy.inference_form) != ("split", 16):
        return "the policy runs a non-default inference form %r (CAVOID_POLICY_F32 / CAVOID_POLICY_PRODUCTS at its creation)" % (
            tuple(policy.inference_form),)
    if int(policy.max_others) != int(env.max_other):
        return "the policy observes %d neighbours, the env's rows carry %d" % (int(policy.max_others), int(env.max_other))
    if frozen_policy is None:
        return "no frozen_policy (fused_crowd=True / cavoid_crowd_eval_run is the one-network form of this launch)"
    fz = frozen_policy
    if not hasattr(fz, "inference_form") or getattr(fz, "_h", None) is None:
        return "the frozen policy is not a FusedPolicy"
    if getattr(fz, "ws", False) or getattr(fz, "arch", "rnn") != "rnn":
        return "the frozen policy is the %s network (the crowd mix evaluation kernel embeds the LSTM pass twice)" % (getattr(fz, "arch", "weight_sharing"),)
    if tuple(fz.inference_form) != ("split", 16):
        return "the frozen policy runs a non-default inference form %r (CAVOID_POLICY_F32 / CAVOID_POLICY_PRODUCTS at its creation)" % (
            tuple(fz.inference_form),)
    if int(fz.max_others) != int(policy.max_others):
        return "the frozen policy observes %d neighbours, the policy %d" % (int(fz.max_others), int(policy.max_others))
    if int(getattr(fz, "num_actions", 0)) != int(getattr(policy, "num_actions", 0)):
        return "the frozen policy has %d actions, the policy %d" % (int(getattr(fz, "num_actions", 0)), int(getattr(policy, "num_actions", 0)))
    return None


class _EvalRecords(object):
    """The device-side records of ``cavoid_eval_run`` for one env, and the per-step outputs it writes (``cavoid_eval_buffers``)."""

    def __init__(self, env: BatchedCollisionAvoidanceEnv):
        W, N, dev = env.num_worlds, env.max_agents, env.device
        self.ret = torch.zeros(W * N, dtype=torch.float64, device=dev)
        self.goal_step = torch.zeros(W * N, dtype=torch.int32, device=dev)
        self.world_steps = torch.zeros(W, dtype=torch.int32, device=dev)
        self.worlds_running = torch.zeros(1, dtype=torch.int32, device=dev)
        self.actions = torch.zeros(W * N, dtype=torch.int32, device=dev)
        self.values = torch.zeros(W * N, dtype=torch.float32, device=dev)
        b = _lib.CavoidEvalBuffers()
        b.struct_size = C.sizeof(_lib.CavoidEvalBuffers)
        b.ret, b.goal_step = self.ret.data_ptr(), self.goal_step.data_ptr()
        b.world_steps, b.worlds_running = self.world_steps.data_ptr(), self.worlds_running.data_ptr()
        self.c = b

    def zero(self) -> None:
        self.ret.zero_(); self.goal_step.zero_(); self.world_steps.zero_()


def _eval_launch(symbol: str, frozen: str, env: BatchedCollisionAvoidanceEnv, policy, frozen_policy, rec: _EvalRecords, n_steps: int, greedy: bool) -> None:
    """One launch of the library's evaluation entry point ``symbol`` on the env's own output buffers (``env.obs`` holds the current
    observation).  ``frozen``: the entry point takes the frozen network's handle, which may be None ("optional"), takes it and needs one
    ("required"), or carries one network and has no such argument ("none")."""
    ptr = lambda t: C.c_void_p(t.data_ptr())
    handles = (env._h, policy._h) + (() if frozen == "none" else (frozen_policy._h if frozen_policy is not None else None,))
    _lib.check(getattr(_lib.lib(), symbol)(*handles, C.byref(rec.c), ptr(env.obs), ptr(env.rewards), ptr(env.done), ptr(env.game_over), ptr(rec.actions),
                                           ptr(rec.values), int(n_steps), 1 if greedy else 0, env._stream()), symbol)


def eval_run(env: BatchedCollisionAvoidanceEnv, policy, frozen_policy, rec: _EvalRecords, n_steps: int, greedy: bool = True) -> None:
    """One ``cavoid_eval_run`` launch on the env's own output buffers (``env.obs`` holds the current observation)."""
    _eval_launch("cavoid_eval_run", "optional", env, policy, frozen_policy, rec, n_steps, greedy)


def eval_run_ws(env: BatchedCollisionAvoidanceEnv, policy, frozen_policy, rec: _EvalRecords, n_steps: int, greedy: bool = True) -> None:
    """One ``cavoid_eval_run_ws`` launch (the weight_sharing network's evaluation kernel): ``eval_run``'s arguments and buffers."""
    _eval_launch("cavoid_eval_run_ws", "optional", env, policy, frozen_policy, rec, n_steps, greedy)


def eval_run_crowd(env: BatchedCollisionAvoidanceEnv, policy, frozen_policy, rec: _EvalRecords, n_steps: int, greedy: bool = True) -> None:
    """One ``cavoid_crowd_eval_run`` launch (the evaluation kernel of crowd worlds): ``eval_run``'s arguments and buffers; the launch
    carries one network, so ``frozen_policy`` must be None."""
    if frozen_policy is not None:
        raise ValueError("cavoid_crowd_eval_run carries one network: no frozen_policy")
    _eval_launch("cavoid_crowd_eval_run", "none", env, policy, None, rec, n_steps, greedy)


def eval_run_crowd_ws(env: BatchedCollisionAvoidanceEnv, policy, frozen_policy, rec: _EvalRecords, n_steps: int, greedy: bool = True) -> None:
    """One ``cavoid_crowd_eval_run_ws`` launch (the evaluation kernel of crowd worlds with the weight_sharing network): ``eval_run_ws``'s
    arguments and buffers."""
    _eval_launch("cavoid_crowd_eval_run_ws", "optional", env, policy, frozen_policy, rec, n_steps, greedy)


def eval_run_crowd_mix(env: BatchedCollisionAvoidanceEnv, policy, frozen_policy, rec: _EvalRecords, n_steps: int, greedy: bool = True) -> None:
    """One ``cavoid_crowd_eval_run_mix`` launch (the evaluation kernel of crowd worlds with a second, frozen ``rnn`` network): ``eval_run``'s
    arguments and buffers; ``frozen_policy`` is required."""
    if frozen_policy is None:
        raise ValueError("cavoid_crowd_eval_run_mix carries two networks: it needs a frozen_policy")
    _eval_launch("cavoid_crowd_eval_run_mix", "required", env, policy, frozen_policy, rec, n_steps, greedy)


def _fused_switches():
    """The fused forms of ``evaluate``: (switch name, reason function, launch).  Read at each call, so that the module's current
    ``eval_run*`` and reason functions are the ones used."""
    return (("fused", evaluate_fused_unavailable_reason, eval_run),
            ("fused_ws", evaluate_fused_ws_unavailable_reason, eval_run_ws),
            ("fused_crowd", evaluate_fused_crowd_unavailable_reason, eval_run_crowd),
            ("fused_crowd_ws", evaluate_fused_crowd_ws_unavailable_reason, eval_run_crowd_ws),
            ("fused_crowd_mix", evaluate_fused_crowd_mix_unavailable_reason, eval_run_crowd_mix))


def _fused_round(env: BatchedCollisionAvoidanceEnv, policy, frozen_policy, rec: _EvalRecords, launch: Callable, steps_per_launch: int, limit: int,
                 greedy: bool) -> Tuple[int, torch.Tensor, torch.Tensor, torch.Tensor]:
    """One round (the env has just been reset) as launches of ``launch`` (``eval_run`` or ``eval_run_ws``): the round's step count, the
    flags it ends with, the returns and the goal steps."""
    rec.zero()
    steps = 0
    while steps < limit:                                   # the last launch is cut so that no world takes more than `limit` steps
        n = min(steps_per_launch, limit - steps)
        launch(env, policy, frozen_policy, rec, n, greedy)
        steps += n
        if int(rec.worlds_running.item()) == 0:            # ONE 4-byte read per launch
            break
    step = int(rec.world_steps.max())                      # = the step-by-step loop's count: the slowest world's
    fl = _settle_finished(env, rec.world_steps, step)
    return step, fl, rec.ret.clone(), rec.goal_step.clone()


def _settle_finished(env: BatchedCollisionAvoidanceEnv, world_steps: torch.Tensor, env_steps: int) -> torch.Tensor:
    """The world buffer the step-by-step loop would have left, and its flags.  That loop goes on stepping worlds that are over until the
    slowest one is, and the first such step leaves a trace in a finished world (``cavoid_step`` latches CAVOID_F_WAS_AT_GOAL /
    _WAS_IN_COLL on an agent that was done before the step and stops it; later ones change nothing).  The kernel takes no step on a
    finished tile, so the worlds that were over before the round's last step take that one step here -- the library's own
    ``cavoid_step``, once per round -- and the worlds that ended AT the last step (or were cut at ``max_steps``) are put back as they
    were: the env is handed back as the loop hands it back."""
    W, N = env.num_worlds, env.max_agents
    before = env.get_state()
    late = world_steps < env_steps
    if not bool(late.any()):
        return before[2]
    env.step(torch.zeros((W, N), dtype=torch.int32, device=env.device))       # (a finished agent ignores what it is given)
    after = env.get_state()
    m = late.repeat_interleave(N)
    merged = [torch.where(m, a, b) for a, b in zip(after, before)]
    env.set_state(*merged)
    return merged[2]


@torch.no_grad()
def evaluate(env: BatchedCollisionAvoidanceEnv, policy: Callable, rounds: int = 1, greedy: bool = True,
             max_steps: Optional[int] = None, frozen_policy=None, fused: bool = False, steps_per_launch: int = 16,
             details: bool = False, fused_ws: bool = False, fused_crowd: bool = False, fused_crowd_mix: bool = False,
             fused_crowd_ws: bool = False) -> Dict[str, float]:
    """Run ``rounds`` batches of ``env.num_worlds`` episodes.  ``policy``: a ``FusedPolicy`` (its ``act`` is used) or any
    callable ``x [B, NN_INPUT_SIZE] -> (p [B, A], v [B])``.  Returns rates over the learning agents that took part.

    ``fused=True`` runs each round on ``cavoid_eval_run`` in launches of ``steps_per_launch`` env steps (raises with
    ``evaluate_fused_unavailable_reason`` where the kernel does not apply); the host reads one word per launch.  Same numbers, with
    one difference in ``mean_reward`` / ``per_agent["ret"]``: the kernel's return stops at the step at which the agent's world is
    over, the loop's goes on summing what ``cavoid_step`` pays finished worlds until the slowest world ends (``reward_time_step``
    where one is set; at the default rewards the getting-close penalty of an agent that ran out of time beside another).
    ``fused_ws=True`` is the same for a ``FusedPolicy`` of the ``weight_sharing`` network: ``cavoid_eval_run_ws``, the same launch loop
    and the same numbers (raises with ``evaluate_fused_ws_unavailable_reason``).  ``fused_crowd=True`` is the same for crowd worlds
    (17 to 64 agents per world) and the ``rnn`` network: ``cavoid_crowd_eval_run``, the ring form of the policy pass and the crowd env step
    per tile (raises with ``evaluate_fused_crowd_unavailable_reason``; no ``frozen_policy``).  ``fused_crowd_ws=True`` is the same for crowd
    worlds and a ``FusedPolicy`` of the ``weight_sharing`` network on either handle (1 to 63 observed neighbours): ``cavoid_crowd_eval_run_ws``,
    the ring form of the weight_sharing pass on the tile's rows that still need an action and the crowd env step per tile, with a
    ``frozen_policy`` of the same kind for frozen-network agents (raises with ``evaluate_fused_crowd_ws_unavailable_reason``).
    ``fused_crowd_mix=True`` is ``fused_crowd=True`` with a ``frozen_policy`` (a ``FusedPolicy`` of the ``rnn`` network, required):
    ``cavoid_crowd_eval_run_mix``, which runs the ring pass once more on the frozen network for the tile's running frozen-network agents
    (raises with ``evaluate_fused_crowd_mix_unavailable_reason``).  The five
    exclude each other; all are opt-in.  A sampled evaluation (``greedy=False``) of SEVERAL rounds on a fused path draws other numbers than
    the step-by-step path from the second round on (every launch advances the policy's step counter, which keys the draw, by its whole
    ``steps_per_launch``, the loop by the steps the round took), as on the other fused paths; one round draws the same.
    ``details=True`` adds ``extra_time_p75`` / ``_p90`` and ``per_agent`` (``reduce_outcomes``)."""
    rec, launch = None, None
    wanted = {"fused": fused, "fused_ws": fused_ws, "fused_crowd": fused_crowd, "fused_crowd_ws": fused_crowd_ws, "fused_crowd_mix": fused_crowd_mix}
    on = [row for row in _fused_switches() if wanted[row[0]]]
    if len(on) > 1:
        raise ValueError("evaluate: " + " and ".join("%s=True" % row[0] for row in on) + " exclude each other (each is one launch form of the round)")
    if on:
        which, reason, launch = on[0]
        why = reason(env, policy, frozen_policy)
        if why is not None:
            raise ValueError("evaluate(%s=True) does not apply: " % which + why)
        if int(steps_per_launch) < 1:
            raise ValueError("steps_per_launch must be >= 1")
        rec = _EvalRecords(env)
    W, N = env.num_worlds, env.max_agents
    dt = float(env.cfg.dt)
    limit = max_steps if max_steps is not None else 100000
    done_rounds = []
    for _ in range(rounds):
        obs = env.reset()
        state0 = env.get_state()
        if launch is not None:
            step, fl, ret, goal_step = _fused_round(env, policy, frozen_policy, rec, launch, int(steps_per_launch), limit, greedy)
        else:
            goal_step = torch.zeros(W * N, dtype=torch.int32, device=env.device)
            ret = torch.zeros(W * N, dtype=torch.float64, device=env.device)
            step = 0
            for step in range(1, limit + 1):
                x = obs.view(W * N, -1)[:, 1:]
                if hasattr(policy, "act"):
                    actions = policy.act(x, greedy=greedy)[0]
                else:
                    p = policy(x.contiguous())[0]
                    actions = p.argmax(dim=1) if greedy else torch.multinomial(p, 1).squeeze(1)
                actions = actions.to(torch.int32).contiguous()
                if frozen_policy is not None:                  # frozen-network agents (scripted policy 4) take their own network's argmax
                    frozen_policy.act(x, greedy=True, rows=env.policy_rows(_lib.POLICY_FROZEN_NET), actions_out=actions)
                obs, rew, done, over = env.step(actions.view(W, N))
                ret += rew.view(-1).double()
                fl = env.get_state()[2]
                now = ((fl & _lib.F_AT_GOAL) != 0) & (goal_step == 0)
                goal_step[now] = step
                if bool(over.all()):
                    break
            fl = env.get_state()[2]
        done_rounds.append({"ret": ret, "goal_step": goal_step, "env_steps": step, "state0": state0, "flags_end": fl})
    return reduce_outcomes(done_rounds, dt, float(env.cfg.near_goal_threshold), details=details)
