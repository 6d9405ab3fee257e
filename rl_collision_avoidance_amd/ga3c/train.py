"""``python -m rl_collision_avoidance_amd.ga3c.train`` -- the GA3C training loop with every actor on the device
(BASELINE configs[4]).  What ``Server.main()`` + 32 ``ProcessAgent`` + 2 ``ThreadPredictor`` + 2 ``ThreadTrainer``
do in the reference (/root/reference/ga3c/GA3C/Server.py:129-170) as ONE loop per GPU:

    hipGraph replay  (policy forward -> sampling -> env.step -> experience bookkeeping, k steps)
    drain rows       -> A3C loss / Adam step (gradients all-reduced over RCCL when launched with torchrun)
    drain episodes   -> the reference's stats line

Multi-GPU: ``python -m torch.distributed.run --nproc-per-node 8 -m rl_collision_avoidance_amd.ga3c.train ...``;
worlds are sharded (globally keyed RNG), the policy is replicated, one flat gradient all-reduce per step."""
from __future__ import annotations

import argparse
import os
import time

import torch
import torch.distributed as dist

from .._lib import TILE_MAX_AGENTS
from ..batched_env import BatchedCollisionAvoidanceEnv
from ..config import EnvConfig
from ..sharding import shard_range
from .network import A3CTrainer, NetworkVP_rnn
from .policy_kernel import (MAX_OTHERS as POLICY_MAX_OTHERS, MAX_OTHERS_INFERENCE as POLICY_MAX_OTHERS_INFERENCE, MAX_OTHERS_WS as POLICY_MAX_OTHERS_WS,
                            MAX_OTHERS_TRAIN as POLICY_MAX_OTHERS_TRAIN, MAX_OTHERS_WS_CROWD as POLICY_MAX_OTHERS_WS_CROWD, FusedA3CTrainer,
                            FusedPolicy)
from .rollout import BatchedRollout
from .stats import EpisodeStats


def save_checkpoint(directory: str, episode: int, net: NetworkVP_rnn, trainer: A3CTrainer) -> str:
    """``NetworkVPCore.save(episode)`` (:235-236): ``<dir>/network_%08d`` -- here a torch file with the variables under
    their TensorFlow names' attributes, the Adam state and the episode count."""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, "network_%08d.pt" % episode)
    torch.save({"episode": int(episode), "model": net.state_dict(), "optimizer": trainer.opt.state_dict(),
                "training_step": trainer.training_step, "arch": net.arch, "max_others": net.max_others}, path)
    return path


def load_checkpoint(path: str, net: NetworkVP_rnn, trainer: A3CTrainer, device) -> int:
    """``NetworkVPCore.load`` (:238-262): returns the episode number the run resumes from."""
    if path.endswith(".npz"):                                  # {TF variable name: array}, see network.load_tf_variables
        import numpy as np
        from .network import load_tf_variables
        load_tf_variables(net, dict(np.load(path)))
        return 0
    ck = torch.load(path, map_location=device)
    # (checkpoints of earlier versions carry no arch / max_others: what their tensors say stands in)
    arch = ck.get("arch", "weight_sharing" if "other_kernel" in ck["model"] else "rnn")
    m = ck.get("max_others")
    if m is None and arch == "weight_sharing":
        m = (ck["model"]["layer1_kernel"].shape[0] - NetworkVP_rnn.HOST) // NetworkVP_rnn.HIDDEN
    if arch != net.arch or (m is not None and int(m) != net.max_others):
        raise SystemExit("%s holds a %s network observing %s neighbours; this run builds a %s network observing %d (--arch / --observed)"
                         % (path, arch, m if m is not None else "?", net.arch, net.max_others))
    # (the optimiser's kind: an entry without one is torch.optim.Adam's state dict, whichever trainer tail wrote it)
    kind, mine = ck.get("optimizer", {}).get("kind", "adam"), getattr(trainer, "optimizer", "adam")
    if "optimizer" in ck and kind != mine:
        raise SystemExit("%s holds the state of the %s optimizer; this run steps with %s (--optimizer)" % (path, kind, mine))
    net.load_state_dict(ck["model"])
    if "optimizer" in ck:
        trainer.opt.load_state_dict(ck["optimizer"])
    trainer.training_step = int(ck.get("training_step", 0))
    return int(ck.get("episode", 0))


# The opt-in one-launch forms of the evaluation round and of the actor loop.  A row: the flag (the first one set wins, in this order), where
# the reason comes from (a function of ga3c.evaluate / a property of BatchedRollout; None: the form applies), the message the run ends with
# where it does not, the line rank 0 prints, and the call (evaluate()'s switch / the BatchedRollout method that captures the launch).
EVALUATE_FORMS = (
    ("fused_evaluate", "evaluate_fused_unavailable_reason",
     lambda why: "--fused-evaluate: the fused evaluation kernel (cavoid_eval_run) does not apply: " + why,
     "[Evaluate] fused evaluation kernel (cavoid_eval_run), %d env steps per launch", "fused"),
    ("fused_ws_evaluate", "evaluate_fused_ws_unavailable_reason",
     lambda why: "--fused-ws-evaluate: the fused weight_sharing evaluation kernel (cavoid_eval_run_ws) does not apply: " + why,
     "[Evaluate] fused weight_sharing evaluation kernel (cavoid_eval_run_ws), %d env steps per launch", "fused_ws"),
    ("fused_crowd_evaluate", "evaluate_fused_crowd_unavailable_reason",
     lambda why: "--fused-crowd-evaluate: the fused crowd evaluation kernel (cavoid_crowd_eval_run) does not apply: " + why,
     "[Evaluate] fused crowd evaluation kernel (cavoid_crowd_eval_run), %d env steps per launch", "fused_crowd"),
    ("fused_crowd_ws_evaluate", "evaluate_fused_crowd_ws_unavailable_reason",
     lambda why: "--fused-crowd-ws-evaluate: the fused crowd weight_sharing evaluation kernel (cavoid_crowd_eval_run_ws) does not apply: " + why,
     "[Evaluate] fused crowd weight_sharing evaluation kernel (cavoid_crowd_eval_run_ws), %d env steps per launch", "fused_crowd_ws"),
    ("fused_crowd_mix_evaluate", "evaluate_fused_crowd_mix_unavailable_reason",
     lambda why: "--fused-crowd-mix-evaluate: the fused crowd evaluation kernel with a frozen network (cavoid_crowd_eval_run_mix) does not apply: " + why,
     "[Evaluate] fused crowd evaluation kernel (cavoid_crowd_eval_run_mix), %d env steps per launch", "fused_crowd_mix"),
)
ACTOR_FORMS = (
    ("fused_crowd_actor", "crowd_fused_unavailable_reason",
     lambda why: "--fused-crowd-actor: the crowd actor kernel (cavoid_crowd_actor_run) does not apply: " + why,
     "fused crowd actor kernel (cavoid_crowd_actor_run), %d env steps per launch", "capture_fused_crowd"),
    ("fused_crowd_mix_actor", "crowd_mix_fused_unavailable_reason",
     lambda why: "--fused-crowd-mix-actor: the crowd actor kernel with a frozen network (cavoid_crowd_actor_run_mix) does not apply: " + why,
     "fused crowd actor kernel (cavoid_crowd_actor_run_mix: learner + frozen network), %d env steps per launch", "capture_fused_crowd_mix"),
    ("fused_ws_actor", "ws_fused_unavailable_reason",
     lambda why: "--fused-ws-actor: the weight_sharing actor kernel (cavoid_actor_run_ws) does not apply: " + why,
     "fused weight_sharing actor kernel (cavoid_actor_run_ws), %d env steps per launch", "capture_fused_ws"),
    ("fused_crowd_ws_actor", "crowd_ws_fused_unavailable_reason",
     lambda why: "--fused-crowd-ws-actor: the crowd weight_sharing actor kernel (cavoid_crowd_actor_run_ws) does not apply: " + why,
     "fused crowd weight_sharing actor kernel (cavoid_crowd_actor_run_ws), %d env steps per launch", "capture_fused_crowd_ws"),
)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--worlds", type=int, default=8192, help="total worlds over all GPUs")
    ap.add_argument("--agents", type=int, default=4, help="MAX_NUM_AGENTS_IN_ENVIRONMENT, 1..64 (4 = TrainPhase1, 10 = TrainPhase2)")
    ap.add_argument("--min-agents", type=int, default=2)
    ap.add_argument("--episodes", type=int, default=20000, help="stop after this many finished episodes (all ranks)")
    ap.add_argument("--steps-per-graph", type=int, default=4)
    ap.add_argument("--scenario-pool", type=int, default=0,
                    help="0 (default): every episode runs the scenario generator; > 0: episodes gather from a pool of that many "
                         "pre-generated scenarios (benchmark aid, NOT the reference's distribution of fresh random test cases)")
    ap.add_argument("--scenario-lookahead", type=int, default=0,
                    help="R > 0 (a power of two > steps per launch; needs --scenario-pool 0): the same fresh scenario per episode, generated by "
                         "the look-ahead refill between launches instead of inside the step (cavoid_cfg::gen_lookahead; bitwise the same run)")
    ap.add_argument("--train-rows", type=int, default=32768,
                    help="rows per Adam step: every drained row is trained on exactly once, in minibatches of this size")
    ap.add_argument("--arch", default="rnn", choices=["rnn", "weight_sharing"],
                    help="MULTI_AGENT_ARCH (Config.py:43-49): the LSTM over the observed agents, or one shared dense filter per slot (the WS-k runs)")
    ap.add_argument("--observed", type=int, default=None, metavar="M",
                    help="MAX_NUM_OTHER_AGENTS_OBSERVED (default: agents - 1; 7 for weight_sharing, Config.py:46-47)")
    ap.add_argument("--sort-method", default=None, choices=["closest_last", "closest_first", "time_to_impact"],
                    help="AGENT_SORTING_METHOD (default: the env config's, closest_last; the recorded WS-k runs use closest_first)")
    ap.add_argument("--torch-policy", action="store_true",
                    help="act with the PyTorch-ROCm graph of the network instead of the fused MFMA kernels")
    ap.add_argument("--autograd-trainer", action="store_true",
                    help="train through PyTorch autograd instead of the fused forward/backward kernels")
    ap.add_argument("--lr", type=float, default=2e-5, help="LEARNING_RATE_RL_START")
    ap.add_argument("--lr-end", type=float, default=None, help="LEARNING_RATE_RL_END (default: no annealing)")
    ap.add_argument("--beta", type=float, default=1e-4, help="BETA_START (entropy regularisation)")
    ap.add_argument("--beta-end", type=float, default=None, help="BETA_END")
    ap.add_argument("--annealing-episodes", type=int, default=None, help="ANNEALING_EPISODE_COUNT (default: --episodes)")
    ap.add_argument("--play", action="store_true", help="PLAY_MODE: argmax actions, trainers disabled (Server.py:134-137)")
    ap.add_argument("--checkpoint-dir", default=None, help="save network_%%08d.pt here (SAVE_MODELS)")
    ap.add_argument("--save-every", type=int, default=50000, help="SAVE_FREQUENCY, in episodes")
    ap.add_argument("--load", default=None, help="checkpoint file to start from (LOAD_CHECKPOINT): a network_%%08d.pt written "
                                                 "by this CLI, or an .npz of the reference's TensorFlow variables by name")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="process-group backend under torchrun (nccl = RCCL over xGMI; gloo only for dry runs)")
    ap.add_argument("--share-device", action="store_true",
                    help="dry run of the multi-rank logic on a 1-GPU box: every rank uses cuda:0 (needs --backend gloo)")
    ap.add_argument("--evaluate", type=int, default=0, metavar="ROUNDS",
                    help="EVALUATE_MODE instead of training: ROUNDS x --worlds episodes with argmax actions, every agent must "
                         "finish; prints success / collision / timeout rates (use with --load)")
    ap.add_argument("--fused-evaluate", action="store_true",
                    help="with --evaluate: run each round as launches of --steps-per-graph env steps of ONE kernel (cavoid_eval_run: policy, "
                         "argmax, env.step without auto-reset and the outcome record per tile of worlds, finished tiles leave early) instead of "
                         "one policy launch, one env launch and one host synchronisation per env step; same numbers.  The run ends if the "
                         "configuration is one the kernel does not carry (crowd worlds, the weight_sharing network, more than 19 observed "
                         "neighbours, the PyTorch policy).  Opt-in (profiles/eval_fused_timing.txt: tools/evalbench.py)")
    ap.add_argument("--fused-ws-evaluate", action="store_true",
                    help="with --evaluate and --arch weight_sharing: the same for the weight_sharing network (up to 16 agents per world and 19 "
                         "observed neighbours) -- launches of --steps-per-graph env steps of cavoid_eval_run_ws (the weight_sharing pass, argmax, "
                         "env.step without auto-reset and the outcome record per tile of worlds); same numbers.  The run ends if the "
                         "configuration is one the kernel does not carry (the rnn network, the ring form above 19 neighbours, crowd worlds, "
                         "the PyTorch policy).  Opt-in (profiles/eval_ws_fused_timing.txt: tools/evalbench.py --arch weight_sharing)")
    ap.add_argument("--fused-crowd-evaluate", action="store_true",
                    help="with --evaluate and --agents 17..64: the same for crowd worlds and the rnn network -- launches of --steps-per-graph env "
                         "steps of cavoid_crowd_eval_run (the ring form of the policy pass, argmax, the crowd env.step without auto-reset and the "
                         "outcome record per tile of floor(64/N) worlds); same numbers.  The run ends if the configuration is one the kernel "
                         "does not carry (up to 16 agents per world, the weight_sharing network, frozen-network agents, holonomic dynamics, the "
                         "PyTorch policy).  Opt-in (profiles/crowd_eval_fused_timing.txt: tools/crowdevalbench.py)")
    ap.add_argument("--fused-crowd-ws-evaluate", action="store_true",
                    help="with --evaluate, --agents 17..64 and --arch weight_sharing: the same for crowd worlds and the weight_sharing network "
                         "(1 to 63 observed neighbours; above 19 with --fused-crowd-ws) -- launches of --steps-per-graph env steps of "
                         "cavoid_crowd_eval_run_ws (the ring form of the weight_sharing pass on the tile's rows that still need an action, argmax, "
                         "the crowd env.step without auto-reset and the outcome record per tile of floor(64/N) worlds; --frozen-policy drives "
                         "frozen-network agents in a second pass); same numbers.  The run ends if the configuration is one the kernel does not "
                         "carry (up to 16 agents per world, the rnn network, holonomic dynamics, the PyTorch policy).  Opt-in "
                         "(profiles/crowd_ws_eval_fused_timing.txt: tools/crowdwsevalbench.py)")
    ap.add_argument("--fused-crowd-mix-evaluate", action="store_true",
                    help="with --evaluate, --agents 17..64 and --frozen-fraction: --fused-crowd-evaluate for worlds with frozen-network agents -- "
                         "launches of --steps-per-graph env steps of cavoid_crowd_eval_run_mix (the ring form of the policy pass, once more on the "
                         "frozen network for the tile's running frozen-network agents, argmax, the crowd env.step without auto-reset and the "
                         "outcome record per tile of floor(64/N) worlds); same numbers.  The run ends if the configuration is one the kernel "
                         "does not carry (up to 16 agents per world, the weight_sharing network, no frozen network, holonomic dynamics, the "
                         "PyTorch policy).  Opt-in (profiles/crowd_mix_timing.txt: tools/crowdmixbench.py)")
    ap.add_argument("--pretrain-steps", type=int, default=0,
                    help="supervised initialisation before RL (the role of Regression.py): Adam steps on teacher-driven rollouts")
    ap.add_argument("--fused-regression", action="store_true",
                    help="run --pretrain-steps on the fused trainer kernels (FusedA3CTrainer.train_regression) where the run trains on them; "
                         "the default stays PyTorch autograd until tools/regbench.py has timed the two against each other "
                         "(profiles/policy_regression_timing.txt)")
    ap.add_argument("--fused-crowd-trainer", action="store_true",
                    help="train rnn networks of 20..64 observed neighbours (--agents 21..64) on the fused ring trainer kernels "
                         "(FusedA3CTrainer(crowd=True)) instead of autograd; opt-in until a whole training run has been timed with and without it "
                         "(profiles/policy_crowd_train_timing.txt holds the trainer step alone: tools/trainbench.py).  --fused-regression then "
                         "takes the supervised start through them too")
    ap.add_argument("--fused-crowd-ws", action="store_true",
                    help="act and train weight_sharing networks of 20..64 observed neighbours (--arch weight_sharing --observed 20..64) on the "
                         "fused weight_sharing ring kernels (FusedPolicy / FusedA3CTrainer with ws_crowd=True) instead of the PyTorch network and "
                         "autograd; opt-in until a whole training run has been timed with and without it (profiles/policy_wsring_timing.txt holds "
                         "one act launch and one trainer step: tools/actbench.py, tools/trainbench.py --arch weight_sharing).  "
                         "--fused-regression then takes the supervised start through them too")
    ap.add_argument("--device-step", action="store_true",
                    help="finish the fused 'rnn' trainer's step inside the HIP library (FusedA3CTrainer(device_step=True): cavoid_policy_weight_grads "
                         "+ cavoid_policy_apply) instead of PyTorch's GEMMs, index_selects and torch.optim.Adam; opt-in (one step with and "
                         "without it: tools/trainbench.py --device-step)")
    ap.add_argument("--ws-device-step", action="store_true",
                    help="the same for the fused 'weight_sharing' trainer (--arch weight_sharing, with or without --fused-crowd-ws; "
                         "FusedA3CTrainer(ws_device_step=True): cavoid_policy_weight_grads_ws + cavoid_policy_apply_ws); opt-in (one step with and "
                         "without it: tools/trainbench.py --ws-device-step)")
    ap.add_argument("--optimizer", default="adam", choices=["adam", "rmsprop"],
                    help="rmsprop: the reference's tf.train.RMSPropOptimizer (decay 0.99, momentum 0.0, epsilon 0.1); needs --device-step "
                         "(--ws-device-step for --arch weight_sharing)")
    ap.add_argument("--grad-clip", type=float, default=None, metavar="C",
                    help="USE_GRAD_CLIP: tf.clip_by_average_norm of every variable's gradient at C (the reference's GRAD_CLIP_NORM is 40); "
                         "needs --device-step (--ws-device-step for --arch weight_sharing)")
    ap.add_argument("--scenario", default="ring", choices=["ring", "box"],
                    help="scenario generator: ring = GEN v1 (antipodal goals on a ring), box = GEN v2 (random starts / goals in a box "
                         "with minimum separations: the shape of the reference's get_testcase_random, TEST_CASE_FN run-ws/config.yaml:281-283)")
    ap.add_argument("--scripted-fraction", type=float, default=0.0,
                    help="P(an agent other than agent 0 runs a scripted policy) -- the reference trained against 'static / non-coop / RVO' "
                         "mixes (checkpoints/RL/wandb/run-2018-backup/checkpoints/index.txt:1-3)")
    ap.add_argument("--static-fraction", type=float, default=0.34, help="of the scripted agents: P(static)")
    ap.add_argument("--rvo-fraction", type=float, default=0.33, help="... P(RVO / ORCA)")
    ap.add_argument("--frozen-fraction", type=float, default=0.0,
                    help="... P(frozen network: a NON-learning agent driven by a frozen NetworkVP_rnn -- the GA3C-CADRL agent, "
                         "Server.py:36); the rest are non-cooperative")
    ap.add_argument("--frozen-policy", default=None,
                    help="checkpoint of the network behind the frozen-network agents (default: a frozen copy of the starting weights)")
    ap.add_argument("--no-actor-kernel", action="store_true",
                    help="run the actors as one launch per phase in a hipGraph instead of the fused actor kernel (cavoid_actor_run)")
    ap.add_argument("--fused-crowd-actor", action="store_true",
                    help="run the actors of crowd worlds (--agents 17..64) as ONE launch per --steps-per-graph env steps (cavoid_crowd_actor_run: "
                         "policy, action draw, env.step and Experience bookkeeping per tile of worlds inside one kernel) instead of one launch "
                         "per phase in a hipGraph; the run ends if the configuration is one the kernel does not carry (frozen-network agents, "
                         "the weight_sharing network, the PyTorch policy).  Opt-in until a whole training run has been timed with and without it "
                         "(profiles/crowd_actor_timing.txt holds the actor loop alone: tools/crowdactorbench.py)")
    ap.add_argument("--fused-crowd-mix-actor", action="store_true",
                    help="--fused-crowd-actor for the training mix with frozen-network agents (--agents 17..64 --scripted-fraction S "
                         "--frozen-fraction F): ONE launch per --steps-per-graph env steps of cavoid_crowd_actor_run_mix, which runs the policy "
                         "pass once more on the frozen network for the tile's running frozen-network agents; the run ends if the configuration "
                         "is one the kernel does not carry (no frozen network, the weight_sharing network, the PyTorch policy).  Opt-in until a "
                         "whole training run has been timed with and without it (profiles/crowd_mix_timing.txt holds the actor loop alone: "
                         "tools/crowdmixbench.py)")
    ap.add_argument("--fused-ws-actor", action="store_true",
                    help="run the actors of the weight_sharing network (--arch weight_sharing, up to 16 agents per world and 19 observed "
                         "neighbours) as ONE launch per --steps-per-graph env steps (cavoid_actor_run_ws: the weight_sharing pass, action draw, "
                         "env.step and Experience bookkeeping per tile of worlds inside one kernel) instead of one launch per phase in a "
                         "hipGraph; the run ends if the configuration is one the kernel does not carry (the rnn network, the ring form above 19 "
                         "neighbours, crowd worlds, frozen-network agents, the PyTorch policy).  Opt-in until a whole training run has been "
                         "timed with and without it (profiles/ws_actor_timing.txt holds the actor loop alone: tools/wsactorbench.py)")
    ap.add_argument("--fused-crowd-ws-actor", action="store_true",
                    help="run the actors of crowd worlds with the weight_sharing network (--agents 17..64 --arch weight_sharing) as ONE launch "
                         "per --steps-per-graph env steps (cavoid_crowd_actor_run_ws: the weight_sharing pass on the rows that need an action, "
                         "action draw, crowd env.step and Experience bookkeeping per tile of worlds inside one kernel) instead of one launch per "
                         "phase in a hipGraph; above 19 observed neighbours it needs --fused-crowd-ws (the policy must be a FusedPolicy on the "
                         "ring kernels); the run ends if the configuration is one the kernel does not carry (the rnn network, tile worlds, "
                         "frozen-network agents, the PyTorch policy).  Opt-in until a whole training run has been timed with and without it "
                         "(profiles/crowd_ws_actor_timing.txt holds the actor loop alone: tools/crowdwsactorbench.py)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--print-every", type=int, default=2000, help="stats line every n episodes (rank 0)")
    ap.add_argument("--faithful-reflush", action="store_true", help="keep the reference's post-done re-flush quirk")
    args = ap.parse_args(argv)

    rank = int(os.environ.get("RANK", "0"))
    size = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.share_device:
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if size > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group("gloo")

    N = args.agents

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            self.TEST_CASE_GENERATOR = args.scenario
            self.SCRIPTED_AGENT_FRACTION = args.scripted_fraction
            self.SCRIPTED_STATIC_FRACTION = args.static_fraction
            self.SCRIPTED_RVO_FRACTION = args.rvo_fraction if args.scripted_fraction > 0 else 0.0
            self.SCRIPTED_FROZEN_NET_FRACTION = args.frozen_fraction if args.scripted_fraction > 0 else 0.0
            if args.observed is not None or args.arch == "weight_sharing":
                self.MAX_NUM_OTHER_AGENTS_OBSERVED = args.observed if args.observed is not None else 7
            EnvConfig.__init__(self)
            if args.sort_method is not None:
                self.AGENT_SORTING_METHOD = args.sort_method
    cfg = Cfg()
    offset, count = shard_range(args.worlds, rank, size)
    # training draws a FRESH scenario for every episode (in-kernel generator, gen_pool_size = 0): the 65 536-entry scenario
    # pool is a latency aid for benchmarks and would make a 20k..2M-episode run revisit a fixed scenario set
    env = BatchedCollisionAvoidanceEnv(count, cfg, device=device, world_offset=offset, seed=1000 * args.seed,
                                       gen_min_agents=min(args.min_agents, N), evaluate_mode=1 if args.evaluate else 0,
                                       gen_pool_size=args.scenario_pool, gen_lookahead=args.scenario_lookahead)
    if rank == 0 and env.cfg.rvo_enabled and N > TILE_MAX_AGENTS:
        print("env: ORCA agents run on the crowd form -- the wavefront solves one agent's programme at a time, one lane per constraint "
              "line (CAVOID_FORM_CROWD_RVO; %d agents per world, P(ORCA | scripted) = %.2f)" % (N, env.cfg.gen_rvo_fraction), flush=True)
    net = NetworkVP_rnn(cfg, seed=args.seed, arch=args.arch).to(device)
    torch_policy, autograd_trainer, crowd_trainer, ws_crowd = args.torch_policy, args.autograd_trainer, False, False
    M = cfg.MAX_NUM_OTHER_AGENTS_OBSERVED
    if net.arch == "weight_sharing":
        if POLICY_MAX_OTHERS_WS < M <= POLICY_MAX_OTHERS_WS_CROWD and args.fused_crowd_ws and not torch_policy and not autograd_trainer:
            # wide weight-sharing rows, opted in: acting and training on the ring kernels (cavoid_policy_wsring.hpp)
            ws_crowd = True
            if rank == 0:
                print("policy: weight_sharing, %d observed neighbours: the fused weight_sharing ring kernel for acting, the fused weight_sharing "
                      "ring trainer kernels for training (%.1f GB of trainer scratch at --train-rows %d)"
                      % (M, FusedA3CTrainer.scratch_bytes(M, FusedA3CTrainer.buffer_rows(args.train_rows), arch="weight_sharing") / 1e9,
                         args.train_rows), flush=True)
        elif M > POLICY_MAX_OTHERS_WS and not (torch_policy and autograd_trainer):
            torch_policy = autograd_trainer = True
            if rank == 0:
                print("policy: the PyTorch network and the autograd trainer -- the fused weight_sharing kernels carry up to %d observed "
                      "neighbours, this run observes %d" % (POLICY_MAX_OTHERS_WS, M), flush=True)
        elif rank == 0:
            print("policy: weight_sharing, %d observed neighbours: %s for acting, %s for training" % (
                M, "the PyTorch network" if torch_policy else "the fused weight_sharing kernel",
                "the autograd trainer" if autograd_trainer else "the fused weight_sharing trainer kernels"), flush=True)
    elif M > POLICY_MAX_OTHERS_INFERENCE and not (torch_policy and autograd_trainer):
        torch_policy = autograd_trainer = True
        if rank == 0:
            print("policy: the PyTorch network and the autograd trainer -- the fused policy kernels carry up to %d observed neighbours, "
                  "this run observes %d" % (POLICY_MAX_OTHERS_INFERENCE, M), flush=True)
    elif M > POLICY_MAX_OTHERS and args.fused_crowd_trainer and not torch_policy and not autograd_trainer and M <= POLICY_MAX_OTHERS_TRAIN:
        # crowd rows, opted in: the fused trainer on the ring kernels (cavoid_policy_train_ring.hpp)
        crowd_trainer = True
        if rank == 0:
            print("policy: the fused crowd policy kernel for acting, the fused ring trainer kernels for training (%d observed neighbours, "
                  "%.1f GB of trainer scratch at --train-rows %d)"
                  % (M, FusedA3CTrainer.scratch_bytes(M, FusedA3CTrainer.buffer_rows(args.train_rows)) / 1e9, args.train_rows), flush=True)
    elif M > POLICY_MAX_OTHERS:
        # crowd rows: fused inference (the crowd kernel) for acting, autograd for training -- the fused trainer parks the whole row
        # (--fused-crowd-trainer: the ring trainer kernels, opt-in -- see the flag's help)
        autograd_trainer = True
        if rank == 0:
            print("policy: %s for acting, the autograd trainer -- the fused trainer carries up to %d observed neighbours, this run observes %d"
                  % ("the PyTorch network" if (torch_policy or net.arch != "rnn") else "the fused crowd policy kernel", POLICY_MAX_OTHERS, M),
                  flush=True)
    fused = None if torch_policy else FusedPolicy(net, seed=1000 * args.seed + rank, ws_crowd=ws_crowd)
    step_flag = "--ws-device-step" if net.arch == "weight_sharing" else "--device-step"
    on_device = args.ws_device_step if net.arch == "weight_sharing" else args.device_step
    if (args.device_step or args.ws_device_step or args.optimizer != "adam" or args.grad_clip is not None) and (
            autograd_trainer or not on_device or (args.device_step and args.ws_device_step)):
        raise SystemExit("--device-step runs behind the fused 'rnn' trainer kernels and --ws-device-step behind the fused 'weight_sharing' ones "
                         "(neither with --autograd-trainer or rows this run trains through autograd), and --optimizer rmsprop / --grad-clip "
                         "need the one of the two that is this network's: %s" % step_flag)
    if autograd_trainer:
        trainer = A3CTrainer(net, learning_rate=args.lr)
    else:
        trainer = FusedA3CTrainer(net, fused, learning_rate=args.lr, crowd=crowd_trainer, ws_crowd=ws_crowd,   # shares (or creates) the packed-weight handle
                                  device_step=args.device_step, optimizer=args.optimizer, grad_clip=args.grad_clip,
                                  ws_device_step=args.ws_device_step)
    if rank == 0 and not args.play:
        if on_device:
            print("trainer tail: cavoid_policy_weight_grads%s + cavoid_policy_apply%s (%s%s) inside the HIP library"
                  % ((("_ws", "_ws") if args.ws_device_step else ("", "")) +
                     (args.optimizer, ", clip_by_average_norm %g" % args.grad_clip if args.grad_clip is not None else "")), flush=True)
        else:
            print("trainer tail: PyTorch (%s, torch.optim.Adam)"
                  % ("autograd" if autograd_trainer else "library GEMMs for the weight gradients"), flush=True)
    episodes_before = 0
    if args.load:
        episodes_before = load_checkpoint(args.load, net, trainer, device)
    def make_frozen():
        """the network behind the frozen-network agents: its own weights (a checkpoint, or a copy of the weights RL starts from --
        loaded or regressed), never trained"""
        if not (args.scripted_fraction > 0 and args.frozen_fraction > 0):
            return None
        most = ((POLICY_MAX_OTHERS_WS_CROWD if ws_crowd else POLICY_MAX_OTHERS_WS) if net.arch == "weight_sharing"
                else POLICY_MAX_OTHERS_INFERENCE)
        if net.max_others > most:
            raise SystemExit("--frozen-fraction needs a FusedPolicy for the frozen network, which carries up to %d observed neighbours "
                             "for the %s network" % (most, net.arch))
        import copy
        frozen_net = copy.deepcopy(net)
        if args.frozen_policy:
            load_checkpoint(args.frozen_policy, frozen_net, A3CTrainer(frozen_net, distributed=False), device)
        for prm in frozen_net.parameters():
            prm.requires_grad_(False)
        return FusedPolicy(frozen_net, seed=0, ws_crowd=ws_crowd)
    if args.evaluate:
        frozen = make_frozen()
        from . import evaluate as evaluation
        if fused is not None:
            fused.refresh(check_range=True)                   # (a checkpoint may have been loaded: a weight beyond the float16 split's range fails loudly)
        eval_policy = fused if fused is not None else net.predict_p_and_v
        form = next((row for row in EVALUATE_FORMS if getattr(args, row[0])), None)
        switch = {}
        if form is not None:
            _, reason, refusal, line, which = form
            why = getattr(evaluation, reason)(env, eval_policy, frozen)
            if why is not None:
                raise SystemExit(refusal(why))
            if args.steps_per_graph < 1:
                raise SystemExit("--steps-per-graph must be >= 1")
            if rank == 0:
                print(line % args.steps_per_graph, flush=True)
            switch = {which: True, "steps_per_launch": args.steps_per_graph}
        res = evaluation.evaluate(env, eval_policy, rounds=args.evaluate, frozen_policy=frozen, **switch)
        if rank == 0:
            print("[Evaluate] " + "  ".join("%s %.4f" % (k, v) if isinstance(v, float) else "%s %d" % (k, v) for k, v in res.items()),
                  flush=True)
        env.close()
        if size > 1:
            dist.destroy_process_group()
        return
    if args.pretrain_steps > 0 and not args.load:
        from .regression import pretrain
        # the supervised start on the fused trainer kernels (train_regression) is opt-in as long as its step is not timed against the
        # autograd step; --autograd-trainer, and every run that falls back to the autograd trainer above, has the autograd path only
        can_fuse = isinstance(trainer, FusedA3CTrainer)
        on_kernels = can_fuse and args.fused_regression
        if rank == 0:
            print("[Regression] on the fused %s trainer kernels" % net.arch if on_kernels else
                  "[Regression] through PyTorch autograd" + (" (the default until the fused %s trainer kernels are timed against it: "
                                                             "--fused-regression runs them)" % net.arch if can_fuse else ""), flush=True)
        info = pretrain(net, env, steps=args.pretrain_steps, log_every=50 if rank == 0 and args.print_every else 0,
                        trainer=trainer if on_kernels else None)
        if size > 1:                                           # every replica starts RL from rank 0's regression result
            for prm in net.parameters():
                dist.broadcast(prm.data, src=0)
        if rank == 0:
            print("[Regression] done: %s" % info, flush=True)
    steps_before = trainer.training_step
    frozen = make_frozen()
    if fused is not None:
        fused.refresh(with_backward=isinstance(trainer, FusedA3CTrainer), check_range=True)      # weights may have come from a checkpoint
    if args.steps_per_graph < 2 or args.steps_per_graph % 2:
        raise SystemExit("--steps-per-graph must be an even number >= 2")
    # the experience ring must hold every block from 'final' (older than TIME_MAX + 2 steps) back to the last drain, i.e.
    # one replay of steps_per_graph steps, plus slack; the re-flush quirk can emit up to one duplicate per slot and step
    time_max = int(getattr(cfg, "TIME_MAX", int(4 / cfg.DT)))
    ring_len = (time_max + 2) + args.steps_per_graph + 8
    roll = BatchedRollout(env, fused if fused is not None else net.predict_p_and_v, reflush_done=args.faithful_reflush,
                          greedy=args.play, ring_len=max(ring_len, 2 * (time_max + 2) + 8), frozen_policy=frozen,
                          dup_capacity=(count * N * (args.steps_per_graph + 1) + 1024) if args.faithful_reflush else None)
    stats = EpisodeStats(print_every=args.print_every if rank == 0 else 0, agents=count)
    anneal_over = args.annealing_episodes or args.episodes
    next_save = episodes_before + args.save_every
    finished = 0
    roll.reset()
    form = next((row for row in ACTOR_FORMS if getattr(args, row[0])), None)
    if form is not None:
        _, reason, refusal, line, capture = form
        why = getattr(roll, reason)
        if why is not None:
            raise SystemExit(refusal(why))
        getattr(roll, capture)(steps_per_graph=args.steps_per_graph)
        actors = line % args.steps_per_graph
    elif roll.fused_available and not args.no_actor_kernel:
        roll.capture_fused(steps_per_graph=args.steps_per_graph)       # K closed-loop steps per launch (cavoid_actor_run)
        actors = "%s, %d env steps per launch" % (roll.actor_path, args.steps_per_graph)
    else:
        roll.capture(steps_per_graph=args.steps_per_graph)
        actors = "%s; in a hipGraph, %d env steps per graph" % (
            roll.actor_path if not roll.fused_available else "one launch per phase (--no-actor-kernel)", args.steps_per_graph)
    if rank == 0:
        print("actors: " + actors, flush=True)
    done_flag = torch.zeros(1, device=device)
    last_loss = None                               # (loss of the last training step -- a device tensor on the fused trainer --, its rows)
    t0 = time.time()
    while True:
        # linear annealing of the learning rate and the entropy weight over the episode count (Server.py:139-147)
        # (a resumed run continues where the checkpoint stopped: Server.py sets episode_count to the loaded episode)
        frac = min(episodes_before + finished, anneal_over - 1) / float(anneal_over)
        trainer.opt.param_groups[0]["lr"] = args.lr + ((args.lr_end if args.lr_end is not None else args.lr) - args.lr) * frac
        net.beta = args.beta + ((args.beta_end if args.beta_end is not None else args.beta) - args.beta) * frac
        roll.replay(1)
        batch = roll.drain(provenance=False)
        if roll.lost_blocks or batch.dropped:      # never train on a silently thinned stream
            raise RuntimeError("rollout lost training rows (%d ring blocks overwritten, %d duplicate rows dropped): "
                               "raise ring_len / dup_capacity or lower --steps-per-graph" % (roll.lost_blocks, batch.dropped))
        # multi-GPU: every rank must enter the same number of gradient all-reduces
        n_chunks = max(1, -(-len(batch) // args.train_rows)) if (len(batch) > 0 or size > 1) else 0
        if args.play:
            n_chunks = 0
        if size > 1:
            done_flag[0] = float(n_chunks)
            dist.all_reduce(done_flag, op=dist.ReduceOp.MAX)
            n_chunks = int(done_flag.item())
        for k in range(n_chunks):
            lo, hi = k * args.train_rows, min((k + 1) * args.train_rows, len(batch))
            lo = min(lo, hi)
            last_loss = (trainer.train(batch.x[lo:hi], batch.r[lo:hi], batch.a_index[lo:hi] if isinstance(trainer, FusedA3CTrainer) else batch.a[lo:hi]),
                         hi - lo)
            stats.add_training_steps(1)
        if fused is not None and n_chunks and not isinstance(trainer, FusedA3CTrainer):
            fused.refresh()                       # the actors see the new weights from the next replay on
            # (the fused trainer re-packs after every optimiser step itself)
        stats.add_episodes(roll.drain_episodes().tolist())
        finished = stats.episode_count
        if size > 1:
            done_flag[0] = float(finished)
            dist.all_reduce(done_flag)
            finished = int(done_flag.item())
        if args.checkpoint_dir and rank == 0 and not args.play and episodes_before + finished >= next_save:
            save_checkpoint(args.checkpoint_dir, episodes_before + finished, net, trainer)      # Server.save_model (:126-127)
            next_save += args.save_every
        if episodes_before + finished >= args.episodes:      # EPISODES counts from the loaded checkpoint on (Server.py:135-147)
            break
    if args.checkpoint_dir and rank == 0 and not args.play:
        save_checkpoint(args.checkpoint_dir, episodes_before + finished, net, trainer)
    if rank == 0:
        dt = time.time() - t0
        print("finished %d episodes in %.1f s: %.0f learning-agent-steps/s per GPU, rolling reward %.4f, %d training steps"
              % (finished, dt, stats.total_frame_count / dt, stats.roll_reward_log, trainer.training_step - steps_before), flush=True)
        if last_loss is not None and last_loss[1] > 0:
            print("last training step: loss %.6g over %d rows" % (float(last_loss[0]), last_loss[1]), flush=True)
    roll.close()
    env.close()
    if size > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
