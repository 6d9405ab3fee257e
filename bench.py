#!/usr/bin/env python
"""bench.py -- agent-steps/s of the batched env.step hot path (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" = one pass of the hot path (decode, dynamics, pairwise sensing, rewards, done flags, sorted
observation, in-kernel restart of finished worlds) over one batch of synthetic worlds: BASELINE
configs[1], 4 agents x 8192 worlds per GPU, unicycle dynamics, random actions pre-generated on the
device; a finished world restarts with a FRESH generator scenario (the reference's reset semantics) from its look-ahead
ring, the refill kernel inside the timed region (`--scenarios pool | instep`: the other sources, all under
extra.scenario_sources).  The K timed steps go through `cavoid_step_autoreset_n`: launches of up to --slices steps, the
world state staying in registers between the steps of a launch; EVERY step reads its action slice and
writes its observations, rewards, done flags and game_over INTO ITS OWN OUTPUT SLOT ([K, W, N, .] tensors:
every step's outputs are there to be read afterwards -- what a rollout consumes, ProcessAgent.py:149-157).
N = 1: no collective.  N > 1 (BASELINE configs[2]: W x N worlds sharded over the GPUs "with a RCCL all-gather of
obs"): every launch writes packed (obs|reward|done) records and their all-gather to every rank
(`cavoid_gather*`, RCCL over xGMI, on its own stream, overlapped with the next launch) is INSIDE the timed
region; the shard-only rate is reported under "extra".  Weak scaling: every rank steps its own 8192 worlds
(RNG keyed on global world ids).  `python bench.py --gpus N` without a launcher starts its own N ranks
(torch.distributed.run, 127.0.0.1).  Rank 0 prints ONE JSON line.

A plain run does only what the headline needs: set-up, pre-roll and warm-up, the timed repetitions of the K steps, --dump-outputs
when given, and the JSON line (metric, value, unit, ms_per_step, timing, config).  `--full` adds everything else the bench measures,
after the timed region: the roofline (HIP-event kernel figures of both launch forms, the null-launch round trip, the device-copy
ceiling, PMC traffic), the N > 1 hand-over forms beside `value`, the configs[3] extra, the other scenario sources, the brief
configs[4] loop, the CPU baselines and the evidence legs (--evidence).  `--sweep` and `--full-loop` add their legs to any run.

N > 1 forms: `--gather all` (default: every rank receives every shard, configs[2]), `--gather root` (only the trainer rank
receives), `--gather none` (shard-only: no exchange); `--gather-every K` = env steps per launch-and-gather block.  Whatever form
`value` is, --full measures the other two briefly in the same run and reports all three under extra.configs2_gather.forms with
their xGMI link figures (bytes per link and step, the link-bound time at 153 GB/s per link and direction, achieved fraction).

roofline (--full): `achieved` / `frac` (= `frac_contract`) are SURVEY section 8d's contract figure -- 192 / 360 algorithmic bytes per
agent-step x the agent-steps of one launch / the launch's HIP-event duration / 8 TB/s; `achieved_moved` / `frac_moved` are priced
on the bytes the timed launch form really moves per agent-step (K-step launch: action in, observation row + reward + done
(+ game_over) out; the world state stays in registers: 117.25 B at N = 4), `traffic` is the PMC measurement of the same
launches, and `one_step_launch` is the same set of figures for the closed-loop form (one step per launch: state in and out
every step).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E vendor peak (MI355X_MICROARCH.md); ~6300 achievable
XGMI_LINK_GBS = 153.0          # one xGMI link, one direction (7 links per GPU, fully connected mesh of 8)


def algorithmic_bytes_per_agent_step(M: int) -> int:
    """SURVEY.md section 8(d), the contract figure: fp32 words -- state read 11 + action 1 + state write 7 + obs (2+4+7M)
    + reward 1 + done 1.  192 B at M=3, 360 B at M=9."""
    return 4 * (11 + 1 + 7 + (6 + 7 * M) + 1 + 1)


def moved_bytes_per_agent_step(M: int, N: int, one_step: bool) -> float:
    """Bytes a launch really has to move per agent-step.  K-step launch (state in registers): action
    4 in; obs row 4(6+7M) + reward 4 + done 1 + game_over 1/N out -- 117.25 B at N=4, 285.1 B at N=10.  One step per launch
    adds the state round trip of the float64 world buffer: read px,py,heading,t (32) + gx,gy,radius,pref (16) + flags 4 +
    episode 4/N, write px,py,heading,t (32) + speed 4 + flags 4 -- 210.25 B at N=4."""
    step = 4 + 4 * (6 + 7 * M) + 4 + 1 + 1.0 / N
    return step + (32 + 16 + 4 + 4.0 / N + 32 + 4 + 4 if one_step else 0.0)


MFMA_PEAK_TFLOPS = 2500.0      # dense f16 / bf16 matrix peak (MI355X_MICROARCH.md); AMD's 5 PF headline includes 2:1 sparsity
F32_VECTOR_PEAK_TFLOPS = 157.3  # float32 vector / f32-input MFMA peak: what a float32-grade predictor is worth against
MFMA_FLOP = 16 * 16 * 32 * 2    # one v_mfma_f32_16x16x32_f16


def split_mfmas_per_wavefront(lstm_steps: float, row_tiles: float = 4.0) -> float:
    """v_mfma_f32_16x16x32_f16 instructions ONE of the four wavefronts of policy_split_tile issues for a 64-row tile
    (csrc/cavoid_policy_split.hpp, the default float16 two-piece form): LSTM step 0 = the input-slot chunk as ONE mixed product over
    4 column tiles x 4 row tiles = 16; every later LSTM step two hidden-state chunks x three partial products + the slot chunk's one
    = 2 x 48 + 16 = 112; layer1 the same 112; layer2 and fullyconnected1 8 chunks x 48 = 384 each; the heads 8 chunks x 3 for the
    wavefront's own row tile.  1144 with three LSTM steps (what SQ_INSTS_MFMA / 2048 wavefronts reads for 32 768 rows).  The fused actor
    kernel computes only `row_tiles` of the four 16-row tiles (the rows that still need an action, packed to the front): every count
    scales with row_tiles / 4 (a head is made by the wavefronts that own a computed row tile)."""
    gemm = 16.0 + 112.0 * max(lstm_steps - 1.0, 0.0) + 112.0 + 384.0 + 384.0
    return (gemm + 24.0) * row_tiles / 4.0


def useful_flop_per_row(M: int, others: float) -> float:
    """multiply-adds x 2 of NetworkVP_rnn inference for one row with `others` observed agents (NetworkVP_rnn.py:58-105): LSTM-64 over 7
    inputs + 64 hidden units per observed agent, layer1 (64 + 4) x 256, layer2 and fullyconnected1 256 x 256, heads 256 x 12"""
    return 2.0 * (others * (7 + 64) * 256 + 68 * 256 + 2 * 256 * 256 + 256 * 12)


def cpu_baseline(N: int, W: int, budget_s: float, pool_size: int):
    """The C float64 oracle (a port/restatement -- the reference env source is absent) timed on this
    box's host cores, 1 thread, on the same workload shape, for about `budget_s` seconds."""
    import numpy as np
    from oracle import c_oracle as co
    cfg, gen = co.default_cfg(N), co.default_gen(N, N, pool_size=pool_size)
    st = co.State.empty(W, N)
    ep = np.zeros(W, np.uint32)
    co.generate(cfg, gen, 0, st, ep)
    rng = np.random.default_rng(0)
    acts = rng.integers(0, 11, size=(16, W, N)).astype(np.int32)
    co.step_autoreset(cfg, gen, 0, st, ep, acts[0])
    n, t0 = 0, time.perf_counter()
    while True:
        co.step_autoreset(cfg, gen, 0, st, ep, acts[n % 16])
        n += 1
        dt = time.perf_counter() - t0
        if dt >= budget_s:
            break
    return {"value": W * N * n / dt, "unit": "agent-steps/s", "cores": 1, "kind": "port",
            "sample": "C float64 oracle (oracle/cavoid_oracle.c), %d agents x %d worlds, %d autoreset steps, %.1f s, 1 thread"
                      % (N, W, n, dt)}


def _fan_out(cmd, procs: int, budget_s: float):
    """`procs` plain subprocesses of `cmd` (nothing is forked from the process that holds the HIP context); each prints its rate
    on its last line.  A straggler is dropped, never waited for beyond the budget + 90 s."""
    import subprocess
    children = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True) for _ in range(procs)]
    vals = []
    deadline = time.time() + budget_s + 90.0
    for ch in children:
        try:
            out, _ = ch.communicate(timeout=max(1.0, deadline - time.time()))
            vals.append(float(out.strip().splitlines()[-1]))
        except Exception:      # noqa: BLE001 -- a straggler must not cost the headline
            ch.kill()
    return vals


def cpu_baseline_all_cores(N: int, W: int, budget_s: float, pool_size: int, max_procs: int = 0):
    """the same C oracle on EVERY host core at once (one process per core -- os.cpu_count() of them -- the
    worlds split evenly: how the reference scales, one env per ProcessAgent process, ProcessAgent.py:221)."""
    procs = max(1, min(max_procs, os.cpu_count() or 1)) if max_procs > 0 else max(1, os.cpu_count() or 1)
    per = max(1, W // procs)
    vals = _fan_out([sys.executable, os.path.abspath(__file__), "--cpu-worker", str(N), str(per), str(budget_s), str(pool_size)], procs, budget_s)
    return {"value": float(sum(vals)), "unit": "agent-steps/s", "cores": len(vals), "host_cpus": os.cpu_count(), "kind": "port",
            "sample": "C float64 oracle, %d processes x %d worlds x %d agents, %.1f s each" % (len(vals), per, N, budget_s)}


def python_baseline_all_cores(N: int, budget_s: float, max_procs: int = 0):
    """the reference-STYLE Python/NumPy oracle (one world object, per-agent objects, Python pair loop) under one
    process per host core, one world per process -- the reference's own parallelism (1 env per ProcessAgent, ProcessAgent.py:221)."""
    procs = max(1, min(max_procs, os.cpu_count() or 1)) if max_procs > 0 else max(1, os.cpu_count() or 1)
    vals = _fan_out([sys.executable, os.path.abspath(__file__), "--py-worker", str(N), str(budget_s)], procs, budget_s)
    return {"value": float(sum(vals)), "unit": "agent-steps/s", "cores": len(vals), "host_cpus": os.cpu_count(), "kind": "port",
            "sample": "oracle/cavoid_oracle.py (reference-style Python objects), %d processes x 1 world x %d agents, %.1f s each"
                      % (len(vals), N, budget_s)}


def python_baseline(N: int, budget_s: float):
    """Reference-style per-object Python/NumPy oracle, one world, one process (baseline B1)."""
    import numpy as np
    from oracle import cavoid_oracle as po
    cfg = po.OracleConfig(max_agents=N, max_other_agents_observed=N - 1)
    gen = po.GenConfig(min_agents=N, max_agents=N)
    rng = np.random.default_rng(0)
    steps, ep, t0 = 0, 0, time.perf_counter()
    world = po.generate_world(0, 0, ep, cfg, gen)
    while time.perf_counter() - t0 < budget_s:
        _, _, over, _ = world.step({i: int(rng.integers(0, 11)) for i in range(N)})
        steps += 1
        if over:
            ep += 1
            world = po.generate_world(0, 0, ep, cfg, gen)
    dt = time.perf_counter() - t0
    return {"value": steps * N / dt, "unit": "agent-steps/s", "cores": 1,
            "sample": "oracle/cavoid_oracle.py, 1 world x %d agents, %d steps" % (N, steps)}


def full_loop(env_cls, cfg, device, W, N, rank, world_size, sync_all, steps: int = 240, train_rows: int = 32768, brief: bool = False):
    """BASELINE configs[4]: everything on the device -- policy inference + action selection (fused f32-MFMA kernel,
    cavoid_policy_*), env.step, experience store / n-step returns (HIP), and Adam steps (PyTorch-ROCm autograd) on
    EVERY drained row, in minibatches of `train_rows` (policy replica per GPU, no collective).  Reports the
    reference's PPS definition: learning-agent steps per second (ProcessStats.py:54-56), for four regimes:
    actors only (PLAY_MODE: no trainer); the full loop with the fused trainer pass (cavoid_policy_train + library
    weight-gradient GEMMs); with the PyTorch autograd trainer; and all-PyTorch (policy and trainer)."""
    import torch
    from rl_collision_avoidance_amd.ga3c.network import A3CTrainer, NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer, FusedPolicy
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    # env steps per launch of the fused actor kernel / per hipGraph replay (even), one hand-over of training rows per launch:
    # 16 -> 405 M, 32 -> 450 M, 64 -> 480 M learning-agent-steps/s actors only (the hand-over and the launch gaps are per launch)
    per_graph = int(os.environ.get("CAVOID_STEPS_PER_GRAPH", "32"))

    def regime(fused: bool, train: bool, fused_trainer: bool = False, actor_kernel: bool = False):
        env = env_cls(W, cfg, device=device, world_offset=rank * W, seed=11)
        net = NetworkVP_rnn(cfg).to(device)
        pol = FusedPolicy(net, seed=rank) if fused else None
        # a policy replica per GPU and NO collective in this extra: ranks drain different row counts, so the number of
        # optimiser steps differs between them
        trainer = FusedA3CTrainer(net, pol, distributed=False) if fused_trainer else A3CTrainer(net, distributed=False)
        # ring: every block from 'final' (older than TIME_MAX + 2 steps) back to the last drain = one replay, plus slack
        time_max = int(getattr(cfg, "TIME_MAX", int(4 / cfg.DT)))
        roll = BatchedRollout(env, pol if fused else net.predict_p_and_v, reflush_done=False,
                              ring_len=max(2 * (time_max + 2) + 8, (time_max + 2) + 2 * per_graph + 10))
        roll.reset()
        if actor_kernel:                                     # the same per_graph steps as ONE launch of the fused actor kernel
            roll.capture_fused(steps_per_graph=per_graph)
        else:
            roll.capture(steps_per_graph=per_graph)          # policy + sampling + env.step + bookkeeping as ONE graph
        rows = [0]

        def run(n_replays):
            # the hand-over of replay k is collected while replay k+1 runs (drain_begin / drain_end): the GPU goes from launch to
            # launch, the host's read-back of the row count is off the critical path
            pending = None

            def consume(b):
                rows[0] += len(b)
                if not train:
                    return
                for lo in range(0, len(b), train_rows):
                    trainer.train(b.x[lo:lo + train_rows], b.r[lo:lo + train_rows],
                                  b.a_index[lo:lo + train_rows] if fused_trainer else b.a[lo:lo + train_rows])
                if pol is not None and len(b) and not fused_trainer:
                    pol.refresh()
            for _ in range(n_replays):
                roll.replay(1)
                h = roll.drain_begin()                       # rows that became training rows (the PPS numerator): compaction enqueued
                if pending is not None:
                    consume(roll.drain_end(pending))
                pending = h
            consume(roll.drain_end(pending))
            return n_replays * per_graph * W * N
        run(8)
        rows[0] = 0
        sync_all()
        t0 = time.perf_counter()
        policy_rows = run(steps // per_graph)
        sync_all()
        dt = time.perf_counter() - t0
        n = (steps // per_graph) * per_graph
        # PPS as the reference counts it (ProcessStats.py:54-56; ProcessAgent.py:237): experiences handed to the trainer.
        # Agents that are done and wait for their world to end still occupy a policy row but yield nothing.
        out = {"learning_agent_steps_per_s_per_gpu": rows[0] / dt, "policy_rows_per_s_per_gpu": policy_rows / dt,
               "ms_per_env_step": dt * 1e3 / n, "env_steps": n, "rows_handed_over": rows[0],
               "training_steps": trainer.training_step if train else 0,
               "actor_path": roll.actor_path if actor_kernel else "one launch per phase (policy, env + bookkeeping) in a hipGraph"}
        if actor_kernel and not train:
            try:
                out["roofline"] = actor_roofline(env, roll, net.max_others)
            except Exception as exc:      # noqa: BLE001 -- a reporting aid
                out["roofline"] = {"error": repr(exc)}
        roll.close()
        env.close()
        return out

    def actor_roofline(env, roll, M):
        """MFMA roofline of actor_kernel<N> (cavoid_actor_run: policy pass + action draw + env.step + Experience bookkeeping per 64-row tile,
        K steps per launch) -- the kernel BASELINE configs[4] runs.  Kernel time: HIP events around launches of `per_graph` steps on the
        launch stream.  Matrix work issued: per tile 4 wavefronts x split_mfmas_per_wavefront(LSTM steps of the tile, row tiles computed) -- the
        kernel packs the rows that still need an action to the front of the tile and computes 2, 3 or 4 of its four 16-row tiles -- counted from
        the live masks at the sampled launch boundaries (a static count of what the kernel's loops issue; the evidence pass replaces it with
        SQ_INSTS_MFMA when it fits the budget).  Useful work: 2 x the network's multiply-adds for the live rows only."""
        live_frac, mf, useful, tiles_by_rt = [], [], [], {0: 0, 2: 0, 3: 0, 4: 0}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        launches, total_ms = 6, 0.0
        for _ in range(launches):
            obs = roll.obs
            flags = env.get_state()[2]
            live = (obs[..., 0] > 0.5) & ((flags.view(W, N) & 7) == 0)             # cavoid_rollout_active_rows' predicate, from the state
            rows = live.reshape(-1)
            pad = (-rows.numel()) % 64
            if pad:
                rows = torch.cat([rows, torch.zeros(pad, dtype=torch.bool, device=rows.device)])
            lens = obs[..., 1].clamp(0, M).reshape(-1)
            if pad:
                lens = torch.cat([lens, torch.zeros(pad, device=lens.device)])
            n_live = rows.view(-1, 64).sum(dim=1)
            steps_t = (lens * rows).view(-1, 64).max(dim=1).values
            rt = torch.where(n_live == 0, torch.zeros_like(n_live), torch.clamp((n_live + 15) // 16, min=2))
            m = 0.0
            for k in (2, 3, 4):
                sel = rt == k
                tiles_by_rt[k] += int(sel.sum().item())
                if bool(sel.any()):
                    st = steps_t[sel]
                    m += float((4.0 * ((16.0 + 112.0 * torch.clamp(st - 1.0, min=0.0) + 112.0 + 768.0 + 24.0) * (k / 4.0))).sum().item())
            tiles_by_rt[0] += int((rt == 0).sum().item())
            mf.append(m)
            live_frac.append(float(live.float().mean().item()))
            useful.append(float((2.0 * (lens[rows] * (7 + 64) * 256 + 68 * 256 + 2 * 256 * 256 + 256 * 12)).sum().item()))
            roll.run_fused(per_graph)                          # (the timed launch is enqueued while this one runs: no host gap inside the event pair)
            ev[0].record()
            roll.run_fused(per_graph)
            ev[1].record()
            torch.cuda.synchronize(device)
            total_ms += ev[0].elapsed_time(ev[1])
            roll.drain(provenance=False)
        us_step = total_ms * 1e3 / (launches * per_graph)
        mfmas = sum(mf) / len(mf)
        issued = mfmas * MFMA_FLOP / us_step * 1e-6
        use = sum(useful) / len(useful) / us_step * 1e-6
        n_t = sum(tiles_by_rt.values())
        return {"kernel": "cavoid::actor_kernel<%d, false, false>" % N, "bound": "mfma", "kernel_us_per_env_step": us_step,
                "steps_per_launch": per_graph, "policy_rows": W * N, "live_row_fraction": sum(live_frac) / len(live_frac),
                "tiles_by_row_tiles_computed": {str(k): v / n_t for k, v in tiles_by_rt.items()},
                "mfma_instructions_per_env_step": mfmas, "mfma_count_source": "static, from the live masks at %d launch boundaries" % launches,
                "issued_TFLOPs": issued, "peak_TFLOPs": MFMA_PEAK_TFLOPS, "frac": issued / MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                "useful_f32_grade_TFLOPs": use, "useful_over_f32_vector_peak": use / F32_VECTOR_PEAK_TFLOPS,
                "note": "issued = matrix instructions x 16 384 flop / kernel time against the dense f16 peak (three partial products per float32 "
                        "product: 3x the useful multiply-adds, on a pipe 16x the float32 rate); useful = the network's own flop for the rows that "
                        "need an action against the 157.3 TF float32 vector / f32-MFMA peak (a ratio above 1 is what the operand split buys: float32-grade results faster than the float32 pipes could make them)"}

    def policy_kernel():
        """The fused inference kernel alone, on real observations: HIP events on the launch stream."""
        env = env_cls(W, cfg, device=device, world_offset=rank * W, seed=11)
        net = NetworkVP_rnn(cfg).to(device)
        pol = FusedPolicy(net, seed=rank)
        obs = env.reset().view(W * N, -1)[:, 1:]
        M = net.max_others

        def timed(fn, n=100):
            for _ in range(10):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize(device)
            return e0.elapsed_time(e1) * 1e3 / n
        fused_us = timed(lambda: pol.act(obs))
        torch_us = timed(lambda: net.predict_p_and_v(obs.contiguous()), 30)
        lens = obs[:, 0].clamp(0, M)
        # The inference kernel computes the float32 GEMMs on v_mfma_f32_16x16x32_f16 by a two-piece float16 operand split, three partial
        # products per float32 product, float32 accumulate (csrc/cavoid_policy_split.hpp; CAVOID_POLICY_PRODUCTS = 3 / 4 / 5: bf16 pieces,
        # that many products; CAVOID_POLICY_F32 = 1: the float32-MFMA kernel).  Reported: the matrix work really ISSUED -- the
        # instructions the kernel executes (split_mfmas_per_wavefront: the same count SQ_INSTS_MFMA reads, checked by the evidence
        # pass below) x 16 384 flop -- against the dense f16 peak, and the useful float32-grade work against the float32 peak.
        steps = lens.view(-1, 64).max(dim=1).values.mean().item() if (W * N) % 64 == 0 else float(M)
        chunks = (1 + 5 * max(steps - 1, 0)) + 5 + 16 + 16 + 1
        flop = W * N * chunks * 16 * 256 * 2
        split = os.environ.get("CAVOID_POLICY_F32", "0") in ("", "0")
        form = int(os.environ.get("CAVOID_POLICY_PRODUCTS", "16"))
        products = 3 if form == 16 else form
        tiles = -(-(W * N) // 64)
        if form == 16:
            mfmas = 4.0 * tiles * split_mfmas_per_wavefront(steps)
        else:                                                   # bf16 forms: every chunk carries `products` products (no mixed slot chunk)
            chunks32 = (1 + 3 * max(steps - 1, 0)) + 3 + 8 + 8
            mfmas = 4.0 * tiles * products * (chunks32 * 16 + 8)
        flop_split = mfmas * MFMA_FLOP
        useful = W * N * useful_flop_per_row(M, float(lens.mean().item()))
        env.close()
        out = {"rows": W * N, "kernel_us": fused_us, "pytorch_graph_us": torch_us}
        if split:
            out.update({"mfma_instructions_per_launch": mfmas, "mfma_instructions_per_wavefront_tile": mfmas / (4.0 * tiles),
                        "mfma_count_source": "static: the kernel's own loop structure (bench.py split_mfmas_per_wavefront)",
                        "issued_TFLOPs": flop_split / fused_us * 1e-6, "peak_TFLOPs": MFMA_PEAK_TFLOPS,
                        "frac": flop_split / fused_us * 1e-6 / MFMA_PEAK_TFLOPS,
                        "useful_f32_grade_TFLOPs": useful / fused_us * 1e-6, "useful_over_f32_vector_peak": useful / fused_us * 1e-6 / F32_VECTOR_PEAK_TFLOPS,
                        "bound": "mfma", "dtype": ("f32 in/out; float16 two-piece split (22-bit operands), %d partial products per float32 product, "
                                                   "f32 accumulate: float32-grade" if form == 16 else
                                                   "f32 in/out; bf16 split, %d partial products per float32 product, f32 accumulate") % products,
                        "precision_vs_float64": ("|dp| <= 1.9e-7, |dv| <= 1.4e-6 incl. x4 inputs (float32-MFMA kernel: 1.8e-7 / 8.7e-7); "
                                                 "profiles/r04_split_f16_vs_bf16.txt") if form == 16 else "|dp| <= 3.7e-6, |dv| <= 2.5e-5 (bf16 pieces)",
                        "kernel": "cavoid::policy_forward_split_duo_kernel (two tiles per workgroup, phases one barrier apart)" if tiles >= 512 and os.environ.get("CAVOID_POLICY_FORM") in (None, "duo")
                                  else "cavoid::policy_forward_split_kernel"})
        else:
            out.update({"issued_TFLOPs": flop / fused_us * 1e-6, "peak_TFLOPs": F32_VECTOR_PEAK_TFLOPS, "frac": flop / fused_us * 1e-6 / F32_VECTOR_PEAK_TFLOPS,
                        "bound": "mfma", "dtype": "f32", "kernel": "cavoid::policy_forward_kernel"})
        return out
    # actor_kernel = cavoid_actor_run: policy -> sample -> env.step -> experience push per 64-row tile, K steps per launch, no kernel
    # boundary inside the loop; the *_graph regimes run the same steps as one launch per phase (5 launches per env step) in a hipGraph
    # BASELINE configs[4] = "4-agent batched env + NetworkVP_rnn policy inference on-device": the ACTORS-ONLY figures.  The trainer legs (loss,
    # backward, Adam on every drained row) are beyond configs[4] and outside SURVEY section 8 (section 2 rows 5 / 7): reported, labelled so.
    res = {"configs4_is": "actors_only_actor_kernel (env + on-device inference + action draw + Experience bookkeeping, no trainer)",
           "policy_kernel": policy_kernel(),
           "actors_only_actor_kernel": regime(True, False, actor_kernel=True),
           "actors_only_fused_policy": regime(True, False)}
    beyond = {"what": "configs[4]'s loop + a trainer consuming every drained row (forward / loss / backward / Adam): NOT part of configs[4]"}
    beyond["actor_kernel_fused_trainer"] = regime(True, True, True, actor_kernel=True)
    if not brief:                                            # the other trainer / policy combinations take most of the time
        beyond["fused_policy_fused_trainer"] = regime(True, True, True)
        beyond["fused_policy_autograd_trainer"] = regime(True, True)
        beyond["torch_policy_autograd_trainer"] = regime(False, True)
    res["beyond_configs4_with_trainer"] = beyond
    res.update({
           "steps_per_graph": per_graph, "train_rows_per_adam_step": train_rows,
           "policy_dtype": "f32 in/out, float16 two-piece operand split on the matrix pipe, f32 accumulate (float32-grade; the actor kernel carries this form)",
           "note": "one launch of the fused actor kernel (or one hipGraph of per-phase launches) per %d env steps; learning_agent_steps = rows handed "
                   "to a trainer (the reference's PPS numerator); reference PPS datum: 563 (32 procs, laptop CPU)" % per_graph})
    return res


def step_kernel_name(N: int, W: int, spl: int, rvo: bool = False) -> str:
    """Which instantiation cavoid_step_autoreset_n takes (csrc/cavoid_capi.hip, cavoid_launch.hpp).  rvo: the world set holds ORCA agents."""
    if rvo:
        if spl == 1:
            return "cavoid::env_kernel<%d, MODE_STEP_AUTORESET, true> (the ORCA instantiation)" % N
        tiles = -(-W // (64 // N))
        if tiles <= 1024 and W * N <= 131072 and os.environ.get("CAVOID_PIPELINE", "2") != "0":
            return "cavoid::env_pipe_kernel<%d, true> (two-wavefront pipeline per tile, the ORCA instantiation)" % N
        return "cavoid::env_kernel<%d, MODE_STEP_AUTORESET_N|PF, true> (the ORCA instantiations)" % N
    if spl == 1:
        tiles1 = -(-W // (64 // N))
        if tiles1 <= 512 and N in (2, 3, 4, 5, 6, 10) and os.environ.get("CAVOID_QUAD", "-1") != "0":
            return "cavoid::env_quad_kernel<%d> (one step by four cooperating wavefronts per tile)" % N
        return "cavoid::env_kernel<%d, MODE_STEP_AUTORESET, false>" % N
    if W * N > 131072:
        return "cavoid::env_kernel<%d, MODE_STEP_AUTORESET_N, false>" % N
    tiles = -(-W // (64 // N))
    pipe = os.environ.get("CAVOID_PIPELINE", "2")
    if tiles <= 512 and N <= 6 and pipe not in ("0", "1"):
        return "cavoid::env_relay_kernel<%d> (roles on the wavefronts of one workgroup per tile)" % N
    if tiles <= 1024 and pipe != "0":
        return "cavoid::env_pipe_kernel<%d, false> (two-wavefront pipeline per tile)" % N
    return "cavoid::env_kernel<%d, MODE_STEP_AUTORESET_PF, false>" % N


def self_launch(args) -> None:
    """`python bench.py --gpus N` with no launcher around it: start N ranks of this script through
    torch.distributed.run on 127.0.0.1 and pass their output through (rank 0 prints the JSON line)."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")         # dmabuf IPC (RCCL across processes)
    env.setdefault("OMP_NUM_THREADS", "1")
    raise SystemExit(subprocess.call(cmd, env=env))


def pmc_child(args) -> None:
    """Child of `measure_traffic` (runs under `rocprofv3 --pmc ...`): the bench's launch pattern, nothing else."""
    import torch
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.config import EnvConfig
    N, W = args.agents, args.worlds

    class Cfg(EnvConfig):
        def __init__(self):
            self.MAX_NUM_AGENTS_IN_ENVIRONMENT = N
            EnvConfig.__init__(self)
    over = {"gen_min_agents": args.min_agents} if args.min_agents else {}
    if args.scenarios == "lookahead" and not args.min_agents:          # (the headline's scenario source; the configs[3] extra keeps the pool)
        over.update(gen_pool_size=0, gen_lookahead=128 if args.slices + 2 <= 128 else 256)
    elif args.scenarios == "instep" and not args.min_agents:
        over.update(gen_pool_size=0)
    env = BatchedCollisionAvoidanceEnv(W, Cfg(), device="cuda:0", seed=7, **over)
    g = torch.Generator(device="cuda").manual_seed(1234)
    acts = torch.randint(0, env.num_actions, (args.slices, W, N), generator=g, device="cuda", dtype=torch.int32)
    env.reset()
    if args.pmc_child == "mfma":
        # the policy kernel alone and the fused actor kernel (configs[4]) under the matrix-instruction counters
        from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
        from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
        from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
        torch.manual_seed(0)
        net = NetworkVP_rnn(Cfg()).cuda()
        pol = FusedPolicy(net, seed=0)
        obs = env.obs.view(W * N, -1)[:, 1:]
        for _ in range(6):
            pol.act(obs)
        K = int(os.environ.get("CAVOID_STEPS_PER_GRAPH", "32"))
        roll = BatchedRollout(env, pol, reflush_done=False, ring_len=4 * K + 64)
        roll.reset()
        for _ in range(14):                                 # (10 launches past the first wave of episode ends, then the 4 that are read)
            roll.run_fused(K)
            roll.drain(provenance=False)
        torch.cuda.synchronize()
        roll.close()
        env.close()
        return
    slots = env.new_step_slots(args.slices) if args.slices > 1 else None
    done = 0
    while done < args.warmup + args.steps:                  # the K-step form ...
        n = min(args.slices, args.warmup + args.steps - done)
        if args.slices > 1:
            env.step_autoreset_n(acts, n, slots=slots)
        else:
            env.step_autoreset(acts[0])
        done += n
    for _ in range(96 if args.slices > 1 else 0):          # ... and the closed-loop form (one step per launch) in the SAME pass
        env.step_autoreset(acts[0])
    torch.cuda.synchronize()
    env.close()


def rocprof_counters(child_args, counters, timeout_s: float):
    """One `rocprofv3 --pmc <counters>` pass (only --kernel-trace beside it) around `python bench.py --pmc-child ...`; -> {kernel name:
    {counter: [value of every dispatch, in dispatch order]}} or None when rocprofv3 is not usable / the pass did not finish in time."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof) or timeout_s < 5.0:
        return None
    d = tempfile.mkdtemp(prefix="cavoid_pmc_", dir="/tmp")
    cmd = [prof, "--pmc"] + list(counters) + ["--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__)] + child_args
    res = {}
    try:
        subprocess.run(cmd, check=True, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), timeout=timeout_s, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        for path in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
            with open(path) as f:
                rows = list(csv.DictReader(f))
                rows.sort(key=lambda r: int(r.get("Dispatch_Id", 0) or 0))
                for row in rows:                                # per kernel and counter: the values in dispatch order
                    res.setdefault(row["Kernel_Name"], {}).setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
        return res or None
    except Exception:      # noqa: BLE001 -- measurement aid only
        return None
    finally:
        shutil.rmtree(d, ignore_errors=True)


def measure_traffic(N: int, W: int, slices: int, steps: int, timeout_s: float = 150.0, min_agents: int = 0, scenarios: str = "pool"):
    """HBM bytes per launch of the step kernels from the PMC counters, collected live: one `rocprofv3 --pmc` pass per counter
    (FETCH_SIZE and WRITE_SIZE do not fit one pass; only --kernel-trace beside --pmc) around a child that repeats this bench's launch
    pattern -- the K-step form AND the one-step form in the same pass, told apart by kernel name.  Counters are KiB; gfx950 tallies
    128-B read requests as 64 B, so FETCH_SIZE is doubled (MI355X_MICROARCH.md, HBM section).  -> {"k_step": {...}, "one_step": {...}}
    (a form that was not seen is missing), or None when rocprofv3 is not usable here / `timeout_s` (for BOTH passes) ran out."""
    import re
    deadline = time.time() + timeout_s
    per = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        child = ["--pmc-child", "step", "--agents", str(N), "--worlds", str(W), "--slices", str(slices), "--steps", str(steps),
                 "--warmup", str(slices), "--min-agents", str(min_agents), "--scenarios", scenarios]
        res = rocprof_counters(child, [ctr], deadline - time.time())
        if res is None:
            return None
        for name, cs in res.items():
            if ctr not in cs:
                continue
            hit = re.search(r"env_kernel<%d, (\d+)" % N, name)
            if (hit and hit.group(1) == "1") or ("env_quad_kernel<%d>" % N) in name:
                form = "one_step"
            elif (hit and hit.group(1) in ("4", "5")) or ("env_pipe_kernel<%d," % N) in name or re.search(r"env_relay_kernel<%d[,>]" % N, name):
                form = "k_step"
            else:
                continue
            tot = per.setdefault(form, {}).setdefault(ctr, [0.0, 0])
            tot[0] += sum(cs[ctr])
            tot[1] += len(cs[ctr])
    out = {}
    for form, cs in per.items():
        if "FETCH_SIZE" not in cs or "WRITE_SIZE" not in cs:
            continue
        fetch_kib, write_kib = cs["FETCH_SIZE"][0] / cs["FETCH_SIZE"][1], cs["WRITE_SIZE"][0] / cs["WRITE_SIZE"][1]
        out[form] = {"traffic": 2.0 * fetch_kib * 1024.0 + write_kib * 1024.0, "FETCH_SIZE_KiB": fetch_kib, "WRITE_SIZE_KiB": write_kib,
                     "dispatches": min(cs["FETCH_SIZE"][1], cs["WRITE_SIZE"][1]), "steps_per_launch": min(slices, steps) if form == "k_step" else 1,
                     "method": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes) --kernel-trace around `bench.py --pmc-child step`; "
                               "mean per step-kernel dispatch; FETCH_SIZE x2 (gfx950 counts 128-B requests as 64 B)"}
    return out or None


def measure_mfma(N: int, W: int, timeout_s: float):
    """SQ_INSTS_MFMA (+ the matrix pipe's busy cycles) per dispatch of the policy kernel and of the fused actor kernel: one pass"""
    res = rocprof_counters(["--pmc-child", "mfma", "--agents", str(N), "--worlds", str(W), "--slices", "2", "--steps", "2", "--warmup", "0",
                            "--scenarios", "pool"], ["SQ_INSTS_MFMA", "SQ_VALU_MFMA_BUSY_CYCLES", "GRBM_GUI_ACTIVE"], timeout_s)
    if res is None:
        return None
    out = {}
    for key, sub in (("policy_kernel", "policy_forward_split_"), ("actor_kernel", "actor_kernel<")):
        for name, cs in res.items():
            if sub in name and "SQ_INSTS_MFMA" in cs:
                # the actor kernel: the LAST launches only -- the child starts from a reset, and until the first episodes end every row of
                # every tile still needs an action (no row tile is skipped): the steady state is what the bench's loop runs in
                keep = 4 if key == "actor_kernel" else len(cs["SQ_INSTS_MFMA"])
                o = {c: sum(v[-keep:]) / len(v[-keep:]) for c, v in cs.items()}
                o["dispatches"] = len(cs["SQ_INSTS_MFMA"][-keep:])
                o["kernel"] = name.split("(")[0]
                if "SQ_VALU_MFMA_BUSY_CYCLES" in o and o.get("GRBM_GUI_ACTIVE"):
                    # 1024 SIMDs / 8 XCDs: the busy cycles are summed over the SIMDs, GRBM_GUI_ACTIVE over the XCDs
                    o["matrix_pipe_busy"] = o["SQ_VALU_MFMA_BUSY_CYCLES"] / (o["GRBM_GUI_ACTIVE"] * 128.0)
                out[key] = o
    return out or None


DUMP_LIMIT_BYTES = 64 << 20


def write_dump(out_dir: str, arrays: dict) -> None:
    """--dump-outputs: every array as out_dir/<name>.npy in float32 (world_index: float64).  All arrays are indexed by world on their first axis; past
    DUMP_LIMIT_BYTES in all, the same fixed, seeded sample of worlds is kept from each, and its indices go to world_index.npy."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    worlds = next(iter(arrays.values())).shape[0]
    if total > DUMP_LIMIT_BYTES - (1 << 20):
        keep = max(1, worlds * (DUMP_LIMIT_BYTES - (1 << 20)) // (total + 8 * worlds))
        idx = np.sort(np.random.default_rng(0).choice(worlds, size=keep, replace=False))
        arrays = dict({name: a[idx] for name, a in arrays.items()}, world_index=idx.astype(np.float64))
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64 if name == "world_index" else np.float32))


def main() -> None:
    if len(sys.argv) >= 6 and sys.argv[1] == "--cpu-worker":        # child of cpu_baseline_all_cores: no torch, no GPU
        print(cpu_baseline(int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]), int(sys.argv[5]))["value"])
        return
    if len(sys.argv) >= 4 and sys.argv[1] == "--py-worker":         # child of python_baseline_all_cores
        print(python_baseline(int(sys.argv[2]), float(sys.argv[3]))["value"])
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--worlds", type=int, default=8192, help="worlds per GPU")
    ap.add_argument("--agents", type=int, default=4)
    ap.add_argument("--slices", type=int, default=64, help="distinct pre-generated action slices = max steps per launch")
    ap.add_argument("--gather", default="all", choices=["all", "root", "none"],
                    help="N>1: the exchange inside the timed region -- all = every rank receives every shard's packed (obs|reward|done) records "
                         "(configs[2]), root = only rank 0 (the trainer rank) does, none = shard-only")
    ap.add_argument("--no-gather", action="store_true", help="= --gather none")
    ap.add_argument("--gather-every", type=int, default=0,
                    help="N>1: env steps per launch-and-gather block (0 = the largest divisor of --steps that fits --slices)")
    ap.add_argument("--force-rccl", action="store_true",
                    help="N=1: put the exchange inside the timed region too, through a forced ONE-rank RCCL communicator (development: "
                         "executes ncclAllGather / the grouped send-recv on a 1-GPU box)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also measure everything beyond the headline: roofline, the N>1 hand-over forms, configs[3], "
                         "the other scenario sources, the brief configs[4] loop, CPU baselines, evidence legs (trimmed by the --no-* options)")
    ap.add_argument("--sweep", action="store_true", help="add a worlds-per-GPU saturation sweep to the JSON line")
    ap.add_argument("--full-loop", action="store_true",
                    help="also time BASELINE configs[4]: batched env + NetworkVP_rnn policy + rollout bookkeeping + Adam steps")
    ap.add_argument("--cpu-seconds", type=float, default=8.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-full-loop", action="store_true", help="skip the brief configs[4] extra of a --full run")
    ap.add_argument("--no-configs3", action="store_true", help="skip the brief configs[3] (10 agents x 8192 worlds) extra")
    ap.add_argument("--scenarios", default="lookahead", choices=["lookahead", "pool", "instep"],
                    help="where a restarting world's scenario comes from in the HEADLINE: lookahead (default) = a fresh generator scenario per episode -- "
                         "the reference's reset semantics -- from per-world look-ahead rings refilled between launches (cavoid_cfg::gen_lookahead; bitwise the "
                         "in-step generator); pool = a hashed pool of 65536 scenarios pre-generated outside the timed region (rounds 1-4's headline); "
                         "instep = the generator inside the step kernel")
    ap.add_argument("--no-fresh-scenarios", action="store_true",
                    help="skip the brief extra that times the same step under the other scenario sources (and with the box generator GEN v2)")
    ap.add_argument("--no-pmc", action="store_true", help="do not collect roofline.traffic live with rocprofv3 --pmc")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="process-group backend for N>1 (nccl = RCCL over xGMI; gloo only for dry runs of the N>1 code path)")
    ap.add_argument("--share-device", action="store_true",
                    help="dry run: the ranks share the visible devices, rank r on cuda:(r %% devices) (on a 1-GPU box every rank uses cuda:0: "
                         "exercises the multi-rank logic there; needs --backend gloo)")
    ap.add_argument("--rendezvous-only", action="store_true",
                    help="launch / rendezvous / collective check of the N>1 path without touching a GPU (CPU boxes, gloo)")
    ap.add_argument("--pmc-child", default="", choices=["", "step", "mfma"], help=argparse.SUPPRESS)
    ap.add_argument("--evidence", default="auto", choices=["auto", "off", "full"],
                    help="the slow evidence legs -- rocprofv3 --pmc child passes (roofline.traffic, SQ_INSTS_MFMA of the policy / actor kernels) and the "
                         "all-host-cores CPU baselines, part of --full: auto (default) = at N = 1 only, inside a 60 s budget, most important first; off; full = no "
                         "budget, + PMC traffic of the configs[3] extra")
    ap.add_argument("--min-agents", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--reps", type=int, default=31, help="repetitions of the K-step timed region (value = the median one; capped at ~5 s of timed work)")
    ap.add_argument("--no-preroll", action="store_true", help="skip the synchronised pre-roll that takes the batch past its first wave of restarts")
    ap.add_argument("--overwrite-outputs", action="store_true",
                    help="round-2 form: every step of a launch overwrites ONE output slot (only the last step's outputs survive)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the timed path returned at its last step (first repetition: the state after preroll + warmup + K steps, "
                         "the same in every run with the same arguments) as DIR/<name>.npy -- rank 0's view: its own shard of the worlds, "
                         "or with the gather in the timed region the records of all ranks it received")
    args = ap.parse_args()
    if args.pmc_child:
        return pmc_child(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # (the launcher's environment normally has it: dmabuf IPC for RCCL across processes)
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world_size != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world_size))
    if args.rendezvous_only:
        # what every N>1 run does around the timed region, with no GPU in it: rendezvous, barrier, MAX over ranks
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world_size > 1:
            dist.init_process_group("gloo")
            t = torch.tensor([1.0 + rank], dtype=torch.float64)
            dist.barrier()
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            assert float(t.item()) == float(world_size)
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            print(json.dumps({"rendezvous": "ok", "n_gpus": world_size, "backend": "gloo"}), flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    from rl_collision_avoidance_amd.batched_env import BatchedCollisionAvoidanceEnv
    from rl_collision_avoidance_amd.config import EnvConfig
    if args.share_device:
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if world_size > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group("gloo")

    N, W = args.agents, args.worlds

    def scen_over(mode, gen_mode=0):
        """cavoid_cfg overrides of a scenario source (see --scenarios); the look-ahead ring must hold one launch (+1)"""
        ring = 128
        while ring < args.slices + 2:
            ring *= 2
        over = {"lookahead": {"gen_pool_size": 0, "gen_lookahead": ring}, "pool": {}, "instep": {"gen_pool_size": 0}}[mode]
        return dict(over, gen_mode=gen_mode) if gen_mode else dict(over)
    SCEN = scen_over(args.scenarios)
    SCEN_TEXT = {"lookahead": "a finished world restarts with a FRESH generator scenario (the reference's reset semantics: a new random test case per reset) taken from its "
                              "look-ahead ring -- exact (seed, global world, episode) streams, bitwise the in-step generator, the refill launches inside the timed "
                              "region",
                 "pool": "a finished world RESTARTS BY GATHERING one of 65536 scenarios pre-generated outside the timed region",
                 "instep": "a finished world restarts with a FRESH scenario generated inside the step kernel"}

    def cfg_for(n_agents):
        class Cfg(EnvConfig):
            def __init__(self):
                self.MAX_NUM_AGENTS_IN_ENVIRONMENT = n_agents
                EnvConfig.__init__(self)
        return Cfg()

    def sync_all():
        torch.cuda.synchronize(device)
        if world_size > 1:
            dist.barrier()
            torch.cuda.synchronize(device)

    def make(Wl, n_agents=N, **over):
        env = BatchedCollisionAvoidanceEnv(Wl, cfg_for(n_agents), device=device, world_offset=rank * Wl, seed=1000 * 0 + 7, **over)
        g = torch.Generator(device=device)
        g.manual_seed(1234 + rank)
        acts = torch.randint(0, env.num_actions, (args.slices, Wl, n_agents), generator=g, device=device, dtype=torch.int32)
        env.reset()
        return env, acts

    def run_steps(env, acts, k, slots=None):
        """k auto-reset steps in launches of up to T = --slices steps (step t of a launch reads acts[t] and, with `slots`,
        writes its outputs into slot t)."""
        T = acts.shape[0] if slots is None else min(acts.shape[0], slots.steps)
        done = 0
        while done < k:
            n = min(T, k - done)
            env.step_autoreset_n(acts, n, slots=slots)
            done += n

    def form_figures(name, n_agents, Wl, spl, launch_ms, one_step):
        """roofline figures of one launch form: `achieved` / `frac` = SURVEY section 8d's contract bytes, `*_moved` = the bytes it
        really moves"""
        M = n_agents - 1
        moved = moved_bytes_per_agent_step(M, n_agents, one_step) * Wl * n_agents * spl
        contract = algorithmic_bytes_per_agent_step(M) * Wl * n_agents * spl
        achieved = contract / (launch_ms * 1e-3) / 1e9
        achieved_moved = moved / (launch_ms * 1e-3) / 1e9
        return {"kernel": name, "steps_per_launch": spl, "kernel_us": launch_ms * 1e3, "kernel_us_per_step": launch_ms * 1e3 / spl,
                "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                "frac_contract": achieved / HBM_PEAK_GBS,
                "contract_bytes_per_agent_step": algorithmic_bytes_per_agent_step(M), "contract_bytes_per_launch": contract,
                "achieved_moved": achieved_moved, "frac_moved": achieved_moved / HBM_PEAK_GBS,
                "moved_bytes_per_agent_step": moved_bytes_per_agent_step(M, n_agents, one_step), "moved_bytes_per_launch": moved,
                "traffic": None}

    def bound_of(fig, Wl, n_agents):
        """what the evidence says limits the kernel: HBM only when the measured traffic really is most of the pipe"""
        real = fig["traffic"] if fig.get("traffic") else fig["moved_bytes_per_launch"]
        if real / (fig["kernel_us"] * 1e-6) / 1e9 >= 0.5 * HBM_PEAK_GBS:
            return "hbm"
        # <= 2 wavefronts per SIMD: the step is ONE wavefront's dependent float64 chain; beyond that the VALU issue rate
        return "latency" if Wl * n_agents <= 131072 else "valu-issue"

    def kernel_figures(env, acts, n_agents, Wl, k, slots=None):
        """per-launch HIP-event durations of the step kernel, in launches shaped like the timed region's, + the one-step form"""
        spl = min(acts.shape[0], k)
        launch_ms = env.kernel_time_ms(acts, max(k, spl), spl, slots=slots)
        rvo = bool(int(getattr(env.cfg, "rvo_enabled", 0)))
        fig = form_figures(step_kernel_name(n_agents, Wl, spl, rvo), n_agents, Wl, spl, launch_ms, one_step=(spl == 1))
        fig["outputs"] = "per-step slots [K,W,N,.]" if slots is not None else "one slot, overwritten by every step"
        single_ms = env.kernel_time_ms(acts, min(max(k, 64), 256), 1)          # the closed-loop form: one step per launch
        fig["one_step_launch"] = form_figures(step_kernel_name(n_agents, Wl, 1, rvo), n_agents, Wl, 1, single_ms, one_step=True)
        return fig

    # ---- the slow evidence legs share one budget (--evidence): most important first, what does not fit is skipped and named ----
    evidence_on = args.full and (args.evidence == "full" or (args.evidence == "auto" and world_size == 1 and not args.no_pmc))
    evidence = {"mode": args.evidence, "budget_s": None if args.evidence == "full" else 60.0, "spent_s": 0.0, "ran": [], "skipped": []}

    def evidence_left():
        return 1e9 if args.evidence == "full" else max(0.0, evidence["budget_s"] - evidence["spent_s"])

    def evidence_leg(name, need_s, fn):
        """run `fn(seconds it may take)` if the budget still holds `need_s`; its wall time is charged"""
        if not evidence_on or rank != 0:
            return None
        if evidence_left() < need_s:
            evidence["skipped"].append(name)
            return None
        t0 = time.time()
        try:
            out = fn(min(evidence_left(), 150.0))
        except Exception:      # noqa: BLE001 -- measurement aid only
            out = None
        evidence["spent_s"] += time.time() - t0
        evidence["ran" if out is not None else "skipped"].append(name)
        return out

    def add_traffic(fig, n_agents, Wl, min_agents=0, name="pmc_traffic"):
        """PMC traffic of both launch forms, live: ONE pair of rocprofv3 --pmc passes around a child that repeats both launch patterns"""
        pmc = evidence_leg(name, 16.0, lambda left: measure_traffic(n_agents, Wl, fig["steps_per_launch"], max(fig["steps_per_launch"] * 4, 128),
                                                                   timeout_s=left, min_agents=min_agents, scenarios=args.scenarios))
        for form, key in ((fig, "k_step"), (fig["one_step_launch"], "one_step")):
            if fig["steps_per_launch"] == 1 and key == "k_step":
                key = "one_step"
            m = (pmc or {}).get(key)
            if m is not None:
                form["traffic"] = m["traffic"]
                form["traffic_over_moved"] = m["traffic"] / form["moved_bytes_per_launch"]
                form["traffic_GBps"] = m["traffic"] / (form["kernel_us"] * 1e-6) / 1e9
                form["traffic_source"] = m
            form["bound"] = bound_of(form, Wl, n_agents)

    scenario_fallback = None
    try:
        env, acts = make(W, **SCEN)
        if args.scenarios == "lookahead":                     # one launch through the refill path before anything is timed
            run_steps(env, acts, 1, None)
            torch.cuda.synchronize(device)
            env.reset()
    except Exception as exc:      # noqa: BLE001 -- the look-ahead must never cost the contract line: fall back to the pool and say so
        if args.scenarios == "pool":
            raise
        scenario_fallback = "--scenarios %s failed (%r): the headline restarts worlds from the pre-generated pool instead" % (args.scenarios, exc)
        args.scenarios = "pool"
        SCEN = scen_over("pool")
        env, acts = make(W, **SCEN)
    if world_size > 1:                                       # (every rank takes the same source)
        flag = torch.tensor([0 if scenario_fallback is None else 1], dtype=torch.int32, device=device if args.backend == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if int(flag.item()) and scenario_fallback is None:
            scenario_fallback = "another rank could not use --scenarios %s: pool" % args.scenarios
            args.scenarios = "pool"
            SCEN = scen_over("pool")
            env.close()
            env, acts = make(W, **SCEN)
    gather_mode = "none" if args.no_gather else args.gather
    exchange_possible = world_size > 1 or args.force_rccl      # (N = 1: only as a development run through a forced RCCL communicator)
    gather_in_metric = exchange_possible and gather_mode != "none"
    gather_root = 0 if gather_mode == "root" else -1
    slots = None if (args.overwrite_outputs or gather_in_metric) else env.new_step_slots(min(args.slices, max(args.steps, 1)))
    sh = None
    extra = {}
    if scenario_fallback:
        extra["scenario_fallback"] = scenario_fallback
    # Synchronised PRE-ROLL (untimed, before the W warm-up steps the contract names): every world starts its first episode at step 0
    # and no episode can end on its time budget before ~40 steps, so a short --warmup would put a timed region in which NO world
    # restarts in front of the clock.  The pre-roll takes the batch past the first wave of restarts, so that the in-kernel
    # auto-reset (part of env.step's job here) is inside the number whatever --warmup is.
    preroll = 0 if args.no_preroll else max(0, 256 - args.warmup)
    comm_status = None
    # launches of `spl` steps: --gather-every, or the largest divisor of K that fits the action slices (K steps = whole launches)
    spl = args.gather_every if args.gather_every > 0 else max(d for d in range(1, min(args.slices, args.steps) + 1) if args.steps % d == 0)
    spl = max(1, min(spl, args.slices))
    if exchange_possible and args.steps % spl:
        raise SystemExit("--gather-every %d must divide --steps %d (the K timed steps are whole launch-and-gather blocks)" % (spl, args.steps))
    acts_l = acts[:spl].contiguous()

    def run_steps_gather(k):
        blocks = None
        for _ in range(-(-k // spl)):
            blocks = sh.gathered_blocks(sh.step_and_gather(acts_l if spl > 1 else acts_l[0], root=sh._root))   # (waits for it; rank-major views, no copy)
        return blocks

    def coll_device():
        return device if (world_size > 1 and args.backend == "nccl") else "cpu"
    if exchange_possible:
        try:
            # configs[2]: this rank's shard of a (world_size x W)-world env; every launch writes packed records into per-step slots
            # and their gather (to every rank, or to the trainer rank) is begun on the communicator's stream -- launch t+1 runs while
            # gather t is on the wire.  nccl: cavoid_gather* (RCCL behind the C ABI); gloo dry run (CPU tests / --share-device): the
            # same blocks through torch.distributed (ShardedEnv picks the transport from the process group's backend).
            from rl_collision_avoidance_amd.sharding import ShardedEnv
            env.close()
            sh = ShardedEnv(world_size * W, cfg_for(N), device=device, seed=7, force_rccl=True if args.force_rccl else None, **SCEN)
            sh.reset()
            env = sh.env
            run_steps(env, acts, preroll, None)
            if gather_in_metric:
                sh.set_gather(spl, gather_root)
                run_steps_gather(args.warmup)
            else:
                slots = None if args.overwrite_outputs else env.new_step_slots(min(args.slices, max(args.steps, 1)))
                run_steps(env, acts, args.warmup, slots)
            torch.cuda.synchronize(device)                    # (a device fault of the warm-up surfaces here, on this rank)
            failed = None
        except Exception as exc:      # noqa: BLE001 -- a broken exchange must not cost the shard-only number: say so and time that
            failed = repr(exc)
        # (no barrier inside the try: a rank that failed goes straight to the status exchange below, so the FIRST collective after the
        #  set-up is the same one on every rank whatever happened)
        # what every rank's communicator set-up (ncclCommInitRank behind cavoid_comm_create, or the gloo stand-in) came to
        comm_status = [None] * world_size
        if world_size > 1:
            try:
                dist.all_gather_object(comm_status, "ok" if failed is None else failed)
            except Exception as exc:      # noqa: BLE001
                comm_status = ["status exchange failed: %r" % (exc,)]
            # every rank takes the same branch: one rank's failure sends all of them to the shard-only measurement
            flag = torch.tensor([0 if failed is None else 1], dtype=torch.int32, device=coll_device())
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            any_failed = bool(int(flag.item()))
        else:
            comm_status, any_failed = ["ok" if failed is None else failed], failed is not None
        if any_failed:
            extra["configs2_gather"] = {"error": failed or "another rank failed", "comm_init_per_rank": comm_status,
                                        "note": "the exchange failed before the timed region: value is the SHARD-ONLY rate"}
            gather_in_metric, exchange_possible = False, False
            if sh is not None:
                try:
                    sh.close()
                except Exception:      # noqa: BLE001
                    pass
                sh = None
            env, acts = make(W, **SCEN)
            slots = None if args.overwrite_outputs else env.new_step_slots(min(args.slices, max(args.steps, 1)))
            run_steps(env, acts, preroll, slots)
            run_steps(env, acts, args.warmup, slots)
    if sh is None and "configs2_gather" not in extra:
        run_steps(env, acts, preroll, slots)
        run_steps(env, acts, args.warmup, slots)

    # ---- timed region: EXACTLY K steps, barrier + synchronize on both sides, max over ranks; REPEATED, value = the median ----------
    def episodes_started():
        return int(env.episode.to(torch.int64).sum().item())

    # the K steps as launches prepared once (arguments checked and converted outside the clock: BatchedCollisionAvoidanceEnv.prepared_autoreset_n) -- the same
    # launches run_steps() makes, what a rollout loop over fixed buffers would hold on to; the look-ahead refill, when one is due, is inside them as before
    prepared = None
    if not gather_in_metric:
        T_l = acts.shape[0] if slots is None else min(acts.shape[0], slots.steps)
        by_len, prepared = {}, []
        for lo in range(0, args.steps, T_l):                  # (every launch reads the same slices from 0 on, like run_steps: one prepared launch per length)
            n_l = min(T_l, args.steps - lo)
            if n_l not in by_len:
                by_len[n_l] = env.prepared_autoreset_n(acts, n_l, slots=slots)
            prepared.append(by_len[n_l])

    last = {}                                                # what the region's last launch returned (a reference: nothing is copied on the clock)

    def timed_once():
        sync_all()
        t0 = time.perf_counter()
        if gather_in_metric:
            last["out"] = run_steps_gather(args.steps)
        else:
            for launch in prepared:
                last["out"] = launch()
        sync_all()
        dt = time.perf_counter() - t0
        if world_size > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=device if args.backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    def last_step_outputs(out):
        """host float32 copies of the last timed step's outputs: obs [W,N,1+D], rewards [W,N], done [W,N], game_over [W]; with the
        gather in the region, the receiving rank's packed records of all ranks' worlds in global order [total,N,1+D+2] (None elsewhere)"""
        if gather_in_metric:
            return None if out is None else {"packed": torch.cat([b[-1] for b in out], dim=0).float().cpu().numpy()}
        obs, rew, done, go = out
        if slots is not None:                                # per-step slots: the region's last step wrote slot n-1 of the last launch
            n_last = (args.steps - 1) % min(acts.shape[0], slots.steps) + 1
            obs, rew, done, go = obs[n_last - 1], rew[n_last - 1], done[n_last - 1], go[n_last - 1]
        return {name: t.float().cpu().numpy() for name, t in (("obs", obs), ("rewards", rew), ("done", done), ("game_over", go))}

    import gc
    dumped = None
    times, restarts = [], []
    reps = max(1, args.reps) | 1
    r = 0
    gc.collect()
    gc_was_on = gc.isenabled()
    gc.disable()                                             # (no collector pause inside a 45 us timed region; back on below)
    while r < reps:
        before = episodes_started()
        times.append(timed_once())
        restarts.append(episodes_started() - before)
        if r == 0 and args.dump_outputs:
            dumped = last_step_outputs(last["out"])          # (between repetitions, off the clock)
        if r == 0 and reps > 3:                              # bound the whole measurement to ~5 s of timed work (same count on every rank)
            reps = max(3, min(reps, int(5.0 / max(times[0], 1e-9)) + 1)) | 1      # odd: the median is a repetition that really ran
            if world_size > 1:
                t = torch.tensor([reps], dtype=torch.int64, device=device if args.backend == "nccl" else "cpu")
                dist.all_reduce(t, op=dist.ReduceOp.MIN)
                reps = int(t.item()) | 1
        r += 1
    if gc_was_on:
        gc.enable()
    if dumped is not None and rank == 0:
        write_dump(args.dump_outputs, dumped)
    order = sorted(range(len(times)), key=lambda i: times[i])
    mid = order[len(order) // 2]
    elapsed = times[mid]                                     # the MEDIAN repetition (an odd count: a repetition that really ran)
    ms_per_step = elapsed * 1e3 / args.steps
    value = world_size * W * N * args.steps / elapsed
    timing = {"timed_reps": len(times), "ms_per_step_median": ms_per_step, "ms_per_step_mean": sum(times) / len(times) * 1e3 / args.steps, "ms_per_step_min": min(times) * 1e3 / args.steps,
              "ms_per_step_max": max(times) * 1e3 / args.steps, "ms_per_step_first_rep": times[0] * 1e3 / args.steps,
              "restarts_in_timed_region": restarts[mid], "restarts_per_rep_min_max": [min(restarts), max(restarts)],
              "preroll_steps": preroll,
              "host_path": ("the region's launches are prepared once (BatchedCollisionAvoidanceEnv.prepared_autoreset_n: arguments checked and pointers converted outside "
                            "the clock; the same cavoid_step_autoreset_n calls, the look-ahead refill included when one is due) and Python's collector is paused around "
                            "the repetitions") if prepared is not None else "step-and-gather calls through ShardedEnv",
              "note": "each repetition = the K timed steps bracketed by barrier + synchronize; value / ms_per_step = the median repetition; "
                      "restarts = worlds of THIS rank whose episode ended and restarted inside that repetition (in-kernel auto-reset)"}

    # host launch + completion round trip of an (almost) empty kernel on this box: what a K-step region issued as ONE launch pays on
    # top of the kernel, whatever the kernel is
    def null_roundtrip_us():
        x = torch.zeros(1, device=device)
        ts = []
        for i in range(70):
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            x.add_(1.0)
            torch.cuda.synchronize(device)
            if i >= 20:
                ts.append(time.perf_counter() - t0)
        return sorted(ts)[len(ts) // 2] * 1e6

    # ---- --full: roofline of the dominant (only) kernel ------------------------------------------------
    roofline = None
    if args.full:
        if slots is None and not args.overwrite_outputs:
            slots = env.new_step_slots(min(args.slices, max(args.steps, 1)))
        roofline = kernel_figures(env, acts, N, W, args.steps, slots)
        launches = -(-args.steps // min(args.slices, max(args.steps, 1)))
        null_us = null_roundtrip_us()
        wall_us, kern_us = ms_per_step * 1e3, roofline["kernel_us_per_step"]
        roofline["wall_clock"] = {
            "us_per_step": wall_us, "kernel_us_per_step": kern_us, "wall_over_kernel": wall_us / kern_us, "launches_per_repetition": launches,
            "null_launch_roundtrip_us": null_us,
            "explained_us_per_step": kern_us + null_us / args.steps,
            "note": ("within 15 % of the kernel time" if wall_us <= 1.15 * kern_us else
                     "the K = %d timed steps are %d launch(es) bracketed by host synchronisation: the region pays one host launch + completion "
                     "round trip (%.1f us for an empty kernel on this box) on top of %.1f us of kernel -- %.0f %% of the gap; use --steps >= 1000 "
                     "(back-to-back launches) for a wall clock that is the kernel's" % (
                         args.steps, launches, null_us, kern_us * args.steps,
                         100.0 * min(1.0, null_us / max(1e-9, (wall_us - kern_us) * args.steps)))) if not gather_in_metric else
                    "with the gather inside the timed region the wall clock is step + exchange, not the step kernel alone"}

    value_path = sh.gather_form if (sh is not None and gather_in_metric) else "no exchange inside the timed region"
    if sh is not None and args.full:
        # every hand-over form beside the one `value` is: the same K steps, barrier + synchronize on both sides, MAX over ranks,
        # median of 3 -- all (every rank receives), root (the trainer rank receives), none (shard-only, no exchange) -- each with its
        # xGMI link figures, so that a SCALE run shows the three curves and what the wire allows
        try:
            rec = W * N * (env.obs_width + 2) * 4                       # bytes of one rank's packed records per env step
            forms = {}

            def time_form(mode):
                if mode == gather_mode:
                    return elapsed
                if mode == "none":
                    sl = slots if slots is not None else env.new_step_slots(min(args.slices, max(args.steps, 1)))
                    fn = lambda: run_steps(env, acts, args.steps, sl)                  # noqa: E731
                else:
                    sh.set_gather(spl, 0 if mode == "root" else -1)
                    fn = lambda: run_steps_gather(args.steps)                           # noqa: E731
                fn()
                ts = []
                for _ in range(3):
                    sync_all()
                    t0 = time.perf_counter()
                    fn()
                    sync_all()
                    dt = time.perf_counter() - t0
                    if world_size > 1:
                        t = torch.tensor([dt], dtype=torch.float64, device=coll_device())
                        dist.all_reduce(t, op=dist.ReduceOp.MAX)
                        dt = float(t.item())
                    ts.append(dt)
                return sorted(ts)[1]
            for mode in ("all", "root", "none"):
                dt = time_form(mode)
                # busiest link, one direction: all = every rank sends its shard to each peer over that peer's own link; root = each
                # link INTO the trainer rank carries one shard; none = nothing travels
                link_bytes = 0 if (mode == "none" or world_size == 1) else rec
                us = dt * 1e6 / args.steps
                bound_us = link_bytes / (XGMI_LINK_GBS * 1e3)
                forms[mode] = {"agent_steps_per_s": world_size * W * N * args.steps / dt, "ms_per_step": dt * 1e3 / args.steps,
                               "bytes_per_link_per_step": link_bytes, "link_bound_us_per_step": bound_us,
                               "link_GBps_achieved": (link_bytes / (us * 1e-6) / 1e9) if link_bytes else 0.0,
                               "xgmi_frac": (bound_us / us) if link_bytes else None,
                               "bytes_received_per_step": {"all": (world_size - 1) * rec, "root": (world_size - 1) * rec, "none": 0}[mode],
                               "receivers": {"all": "every rank", "root": "rank 0 (the trainer rank)", "none": "nobody"}[mode]}
            rccl = bool(sh._native) and bool(getattr(sh._native, "uses_rccl", False))
            extra["configs2_gather"] = {
                "value_is": gather_mode, "forms": forms,
                "path": value_path,
                "transport": sh.transport, "uses_rccl": rccl, "rccl_version": getattr(sh._native, "rccl_version", 0) if rccl else 0,
                "comm_init_per_rank": comm_status, "steps_per_launch": spl,
                "bytes_sent_per_rank_per_step": rec, "bytes_received_per_rank_per_step": (world_size - 1) * rec,
                "xgmi_link_peak_GBps": XGMI_LINK_GBS,
                "agent_steps_per_s_with_gather": forms["all"]["agent_steps_per_s"], "ms_per_step_with_gather": forms["all"]["ms_per_step"],
                "agent_steps_per_s_shard_only": forms["none"]["agent_steps_per_s"], "ms_per_step_shard_only": forms["none"]["ms_per_step"],
                "note": "xgmi_frac = link-bound time / measured time per step = achieved GB/s on the busiest link / %.0f: what the wire allows is "
                        "(8192 x 4 x 116 B = 3.8 MB per link and step) / 153 GB/s = 24.8 us per env step whatever the form, against ~1.5 us of "
                        "compute -- an every-step hand-over of ALL observations is wire-bound by construction; the shard-only form is the "
                        "env.step scaling curve.  Under --backend gloo / --share-device (dry runs) nothing crosses a link: the figures then "
                        "only exercise the code path.  No multi-GPU run has been made by the builder (1-GPU boxes): the driver's is the first."
                        % XGMI_LINK_GBS}
        except Exception as exc:      # noqa: BLE001 -- report, never lose the headline
            extra["configs2_gather"] = {"error": repr(exc)}

    # "also report vs a measured device-copy ceiling" -- a 1 GiB device-to-device copy on this box (read + write bytes / time)
    def measured_copy_GBps():
        try:
            n = 1 << 28
            a, b = torch.empty(n, dtype=torch.float32, device=device), torch.empty(n, dtype=torch.float32, device=device)
            a.fill_(1.0)
            b.copy_(a)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(device)
            e0.record()
            for _ in range(5):
                b.copy_(a)
            e1.record()
            torch.cuda.synchronize(device)
            del a, b
            return 5 * 2 * n * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9
        except Exception:      # noqa: BLE001 -- a reporting aid
            return None
    if roofline is not None:
        if rank == 0:
            copy_gbps = measured_copy_GBps()
            if copy_gbps:
                roofline["measured_copy_GBps"] = copy_gbps
                roofline["frac_of_measured_copy"] = roofline["achieved"] / copy_gbps
                roofline["one_step_launch"]["frac_of_measured_copy"] = roofline["one_step_launch"]["achieved"] / copy_gbps
        if rank == 0 and evidence_on:
            add_traffic(roofline, N, W)
        for form in (roofline, roofline["one_step_launch"]):
            form.setdefault("bound", bound_of(form, W, N))
        roofline["bound_note"] = ("latency = the dependent float64 chain of the wavefront(s) that own a tile (<= 2 wavefronts per SIMD at this "
                                  "batch size); valu-issue = vector issue rate at saturation; hbm only when the measured traffic exceeds half "
                                  "the 8 TB/s pipe.  `frac` is still the HBM-roofline fraction the contract asks for.")

    if args.full and rank == 0 and not args.no_configs3 and N != 10:
        # BASELINE configs[3] beside the headline: 10 agents (TrainPhase2 shape, 2..10 agents per world, M = 9) x 8192 worlds
        try:
            e3, a3 = make(8192, 10, gen_min_agents=2)
            s3 = None if args.overwrite_outputs else e3.new_step_slots(a3.shape[0])
            run_steps(e3, a3, 256, s3)                      # (past the first, synchronised wave of restarts)
            torch.cuda.synchronize(device)
            t3 = time.perf_counter()
            run_steps(e3, a3, 640, s3)
            torch.cuda.synchronize(device)
            dt3 = time.perf_counter() - t3
            r3 = kernel_figures(e3, a3, 10, 8192, 640, s3)
            if args.evidence == "full":                     # (default runs: profiles/ holds this form's PMC traffic)
                add_traffic(r3, 10, 8192, min_agents=2, name="pmc_traffic_configs3")
            for form in (r3, r3["one_step_launch"]):
                form.setdefault("bound", bound_of(form, 8192, 10))
            c3 = {"workload": "BASELINE configs[3]: 10 agents (2..10 present) x 8192 worlds, M = 9, obs width 69; per-step output slots",
                  "value": 8192 * 10 * 640 / dt3, "unit": "agent-steps/s", "ms_per_step": dt3 * 1e3 / 640, "roofline": r3}
            del s3
            if not args.no_cpu_baseline:
                c3["cpu_baseline"] = cpu_baseline(10, 2048, min(2.0, args.cpu_seconds), int(e3.cfg.gen_pool_size))
            extra["configs3_n10"] = c3
            e3.close()
            del e3, a3
        except Exception as exc:      # noqa: BLE001
            extra["configs3_n10"] = {"error": repr(exc)}

    if args.full and rank == 0 and not args.no_fresh_scenarios:
        # the reference's reset semantics (TEST_CASE_FN = get_testcase_random, run-ws/config.yaml:281-283: a NEW random scenario at every
        # reset, ProcessAgent.py:107): the same K-step timed region with NO scenario pool -- every restart generates its scenario inside the
        # step kernel, exact (seed, global world id, episode) streams -- for GEN v1 (rings) and GEN v2 (boxes, rejection sampling)
        fresh = {}
        # the same K-step timed region under the scenario sources the headline does NOT use (GEN v1 rings), and under GEN v2 (boxes, rejection
        # sampling) with the look-ahead and in the step kernel.  lookahead / instep are the same scenarios bit for bit (tests/test_gpu_lookahead.py).
        cases = [("gen_v1_ring_" + m, scen_over(m)) for m in ("lookahead", "pool", "instep") if m != args.scenarios]
        cases += [("gen_v2_box_" + m, scen_over(m, gen_mode=1)) for m in ("lookahead", "instep")]
        # the reference's TRAINING MIX (static / non-cooperative / ORCA agents around the learners, index.txt:1-3): ORCA agents in the worlds take
        # the two-wavefront pipeline's ORCA instantiation -- the role-split relay kernel with ORCA agents was built and is SLOWER (an ORCA action reads the
        # committed state of its world, so the state owner cannot speculate across it: 12.2 against 7.6 us per step, profiles/r06_ac_relay_rvo.txt) --
        # this is what a training run's env.step costs
        cases += [("training_mix_orca_agents_pool", dict(rvo_enabled=1, gen_rvo_fraction=0.4, gen_nonlearning_fraction=0.5, gen_static_fraction=0.2,
                                                         gen_min_agents=2))]
        n_rep = 3
        for label, over in cases:
            try:
                e0, a0 = make(W, N, **over)
                s0 = None if args.overwrite_outputs else e0.new_step_slots(min(args.slices, max(args.steps, 1)))
                run_steps(e0, a0, preroll + args.warmup, s0)
                ts, rs = [], []
                for _ in range(n_rep):
                    before = int(e0.episode.to(torch.int64).sum().item())
                    torch.cuda.synchronize(device)
                    t0 = time.perf_counter()
                    run_steps(e0, a0, args.steps, s0)
                    torch.cuda.synchronize(device)
                    ts.append(time.perf_counter() - t0)
                    rs.append(int(e0.episode.to(torch.int64).sum().item()) - before)
                mid0 = sorted(range(n_rep), key=lambda i: ts[i])[n_rep // 2]
                f0 = kernel_figures(e0, a0, N, W, args.steps, s0)
                fresh[label] = {"value": W * N * args.steps / ts[mid0], "unit": "agent-steps/s", "ms_per_step": ts[mid0] * 1e3 / args.steps,
                                "restarts_in_timed_region": rs[mid0], "timed_reps": n_rep, "roofline": f0,
                                "vs_headline_kernel_us_per_step": [f0["kernel_us_per_step"], roofline["kernel_us_per_step"]]}
                del s0
                e0.close()
                del e0, a0
            except Exception as exc:      # noqa: BLE001
                fresh[label] = {"error": repr(exc)}
        fresh["headline_source"] = args.scenarios
        fresh["note"] = ("scenario source of a restarting world -- lookahead: a fresh generator scenario per episode (the reference makes a new random test case "
                         "per reset) from per-world rings a small refill kernel tops up between launches (`value` includes the refill, `roofline` is the step "
                         "kernel alone); instep: the same scenarios, bit for bit, generated inside the step kernel; pool: gathered from 65536 scenarios "
                         "pre-generated outside the timed region.  Same K, same per-step output slots as the headline, this rank's GPU only")
        extra["scenario_sources"] = fresh

    if args.full_loop or (args.full and not args.no_full_loop):
        # configs[4] beside the headline (--full: a brief version, actors only + the fused-trainer loop, ~15 s; the PyTorch comparison
        # legs only with --full-loop).  At N > 1 every rank runs it on its own shard and policy replica, concurrently and
        # without any collective; rank 0 reports its own per-GPU figures.
        try:
            extra["full_ga3c_loop"] = full_loop(BatchedCollisionAvoidanceEnv, cfg_for(N), device, W, N, rank, world_size, sync_all,
                                                brief=not args.full_loop, steps=512 if args.full_loop else 256)
        except Exception as exc:      # noqa: BLE001  (an extra must never cost the contract line)
            extra["full_ga3c_loop"] = {"error": repr(exc)}

    if args.sweep and rank == 0:
        sweep = []
        for Ws in (1024, 8192, 65536, 262144, 1048576):
            e2, a2 = make(Ws)
            spl2 = min(a2.shape[0], max(1, (1 << 30) // (Ws * N * (e2.obs_width + 2) * 4)))     # <= 1 GiB of output slots
            a2 = a2[:spl2].contiguous()
            s2 = None if args.overwrite_outputs else e2.new_step_slots(spl2)
            run_steps(e2, a2, spl2, s2)
            f = kernel_figures(e2, a2, N, Ws, 2 * spl2, s2)
            torch.cuda.synchronize(device)
            one = f["one_step_launch"]
            sweep.append({"worlds": Ws, "kernel_us_per_step": f["kernel_us_per_step"], "steps_per_launch": f["steps_per_launch"],
                          "agent_steps_per_s": Ws * N / (f["kernel_us_per_step"] * 1e-6), "GBps": f["achieved"], "frac": f["frac"],
                          "frac_moved": f["frac_moved"], "one_step_launch_us": one["kernel_us"], "one_step_launch_frac": one["frac"],
                          "one_step_launch_frac_moved": one["frac_moved"]})
            e2.close()
            del e2, a2, s2
        extra["saturation_sweep"] = sweep

    which = {4: "configs[1]", 10: "configs[3]"}.get(N, "configs[1]-style")
    line = {
        "metric": "agent-steps/sec (env.step) at %d agents x %d worlds per GPU" % (N, W),
        "value": value, "unit": "agent-steps/s", "n_gpus": world_size, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": "BASELINE %s: %d agents x %d worlds per GPU, unicycle dynamics, GEN v1 synthetic scenarios, "
                               "uniform random actions pre-staged on the device, in-kernel auto-reset -- %s (the other scenario sources, "
                               "GEN v1 and GEN v2, with --full: extra.scenario_sources); launches of up to %d steps "
                               "(world state in registers between the steps of a launch); %s%s"
                               % (which, N, W, SCEN_TEXT[args.scenarios], args.slices,
                                  "every step overwrites one output slot" if args.overwrite_outputs else
                                  "every step's obs / reward / done / game_over written into its own output slot [K,W,N,.]",
                                  ("; + the gather of the packed records to %s inside the timed region (configs[2])"
                                   % ("every rank" if gather_root < 0 else "rank 0, the trainer rank")) if gather_in_metric else ""),
                   "worlds_per_gpu": W, "agents_per_world": N, "obs_width": env.obs_width, "steps_per_launch": min(args.slices, args.steps),
                   "scenarios": args.scenarios,
                   "parallelism": ("worlds sharded over %d GPU(s), one gather of (obs|reward|done) per launch to %s (RCCL over xGMI); value = the "
                                   "with-gather rate (wire-bound: see wire_bound_agent_steps_per_s), scaling is judged on value_shard_only"
                                   % (world_size, "every rank" if gather_root < 0 else "rank 0"))
                                  if gather_in_metric else ("worlds sharded over %d GPU(s), no data-path collective" % world_size)},
        "timing": timing,
    }
    if roofline is not None:
        line["roofline"] = roofline
    if args.full and rank == 0 and world_size == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline(N, W, args.cpu_seconds, int(env.cfg.gen_pool_size))
        line["cpu_baseline"]["host_cpus"] = os.cpu_count()
        extra["python_reference_style_baseline"] = python_baseline(N, min(2.0, args.cpu_seconds))
        # every host core at once: evidence legs -- hundreds of processes, ~10 s each way
        pool_sz = int(env.cfg.gen_pool_size)
        r = evidence_leg("cpu_baseline_all_cores", 12.0, lambda left: cpu_baseline_all_cores(N, W, 2.0, pool_sz))
        if r is not None:
            extra["cpu_baseline_all_cores"] = r
    if rank == 0 and evidence_on and "full_ga3c_loop" in extra and "error" not in extra["full_ga3c_loop"]:
        # SQ_INSTS_MFMA of the policy kernel and of the fused actor kernel: the issued-flop figures from the instructions the hardware counted
        m = evidence_leg("pmc_mfma", 18.0, lambda left: measure_mfma(N, W, left))
        if m:
            fl = extra["full_ga3c_loop"]
            pk = fl.get("policy_kernel", {})
            if "policy_kernel" in m and "kernel_us" in pk and pk.get("bound") == "mfma" and "mfma_instructions_per_launch" in pk:
                n_m = m["policy_kernel"]["SQ_INSTS_MFMA"]
                pk.update({"mfma_instructions_per_launch_static": pk["mfma_instructions_per_launch"], "mfma_instructions_per_launch": n_m,
                           "mfma_count_source": "rocprofv3 --pmc SQ_INSTS_MFMA, mean per dispatch", "issued_TFLOPs": n_m * MFMA_FLOP / pk["kernel_us"] * 1e-6,
                           "frac": n_m * MFMA_FLOP / pk["kernel_us"] * 1e-6 / MFMA_PEAK_TFLOPS, "pmc": m["policy_kernel"]})
            ar = fl.get("actors_only_actor_kernel", {}).get("roofline", {})
            if "actor_kernel" in m and "kernel_us_per_env_step" in ar:
                per_step = m["actor_kernel"]["SQ_INSTS_MFMA"] / ar["steps_per_launch"]
                ar.update({"mfma_instructions_per_env_step_static": ar["mfma_instructions_per_env_step"], "mfma_instructions_per_env_step": per_step,
                           "mfma_count_source": "rocprofv3 --pmc SQ_INSTS_MFMA per dispatch / steps per launch",
                           "issued_TFLOPs": per_step * MFMA_FLOP / ar["kernel_us_per_env_step"] * 1e-6,
                           "frac": per_step * MFMA_FLOP / ar["kernel_us_per_env_step"] * 1e-6 / MFMA_PEAK_TFLOPS, "pmc": m["actor_kernel"]})
    if args.full and rank == 0 and world_size == 1 and not args.no_cpu_baseline:
        r = evidence_leg("python_reference_style_baseline_all_cores", 14.0, lambda left: python_baseline_all_cores(N, 2.0))
        if r is not None:
            extra["python_reference_style_baseline_all_cores"] = r
    if args.full and rank == 0:
        evidence["spent_s"] = round(evidence["spent_s"], 1)
        extra["evidence"] = evidence
    # ---- what `value` is, spelled out at the top level (N > 1: which hand-over form, what the wire allows, what the >= 6x target is judged on) ----
    g2 = extra.get("configs2_gather", {}) if isinstance(extra.get("configs2_gather"), dict) else {}
    forms = g2.get("forms", {})
    rec_bytes = W * N * (env.obs_width + 2) * 4
    line["value_shard_only"] = forms["none"]["agent_steps_per_s"] if "none" in forms else (value if not gather_in_metric else None)
    line["value_gather_all"] = forms["all"]["agent_steps_per_s"] if "all" in forms else None
    line["value_gather_root"] = forms["root"]["agent_steps_per_s"] if "root" in forms else None
    line["value_is"] = gather_mode if gather_in_metric else "shard_only"
    # an every-step hand-over of ALL packed records: each rank's link carries W x N x (1 + D + 2) x 4 bytes per env step, one direction
    line["wire_bound_agent_steps_per_s"] = (world_size * W * N / (rec_bytes / (XGMI_LINK_GBS * 1e9))) if world_size > 1 else None
    line["scaling_judged_on"] = ("value_shard_only: worlds are independent (SURVEY section 8e), so the >= 6x at 8 GPUs target of BASELINE.json is the shard-only "
                                 "env.step curve's to meet; value_gather_all (configs[2]: every rank receives every observation, every step) is bound by the xGMI "
                                 "links at wire_bound_agent_steps_per_s whatever the kernels do -- below ONE GPU's shard-only rate by construction -- and "
                                 "value_gather_root is the trainer-rank form of the same bytes")
    if extra:
        line["extra"] = extra
    if sh is not None:
        sh.close()
    else:
        env.close()
    # ONE JSON line, and the LAST thing on stdout: RCCL prints a version banner through C stdio at its first communicator (buffered when
    # stdout is a pipe or a file, i.e. it would surface at process exit, BEHIND the line) -- every rank flushes its C streams, then a
    # barrier, then rank 0 prints
    def flush_c_stdio():
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:      # noqa: BLE001
            pass
        sys.stdout.flush()
    flush_c_stdio()
    if world_size > 1:
        dist.barrier()
        dist.destroy_process_group()
        flush_c_stdio()
    if rank == 0:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
