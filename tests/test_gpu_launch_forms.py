"""Every K-step launch form of the env step against the plain one-step kernel, bit for bit, and each form proven to have run.

The env step has one plain implementation: env_kernel, one step per launch on one wavefront per tile (CAVOID_QUAD=0), held to the
float64 oracle in test_gpu_parity.py.  The K-step forms copy its arithmetic and must be BIT-identical to it:
  RELAY    env_relay_kernel (CAVOID_PIPELINE=2, CAVOID_RELAY_CONSUMERS=nc): the step cut into roles on 3 + nc wavefronts per tile,
           with its own copies of the advance, the sort keys, the cooperative last step and a 64-step action ring;
  PIPE     env_pipe_kernel (CAVOID_PIPELINE=1), and by fallback where the relay does not carry a configuration (N > 6, U4 flipped);
  LOOP_PF  env_kernel's step loop with the next pool record in registers (CAVOID_PIPELINE=0);
  LOOP     env_kernel's step loop gathering restarts on demand (CAVOID_PREFETCH_POOL=0: out of latency mode).
A launcher that does not carry a configuration hands it to the next form without a word, so every launch here asserts the form
that ran (BatchedCollisionAvoidanceEnv.last_step_form, with the relay's consumer count) -- a silent fallback fails the test.

Per configuration ONE reference env steps one launch per step; beside it every applicable form runs the same actions in launches of
1, 2 ... 6, the relay ring depth +-1, 47 / 48 / 49 (the loader's lead), 63 / 64 / 65 and 100 / 129 steps (the action ring wraps
once and twice), each form three times over: every step into its own slot, every step as packed records, and out_step_stride = 0
(only the last step survives).  After every launch: every slot, the state and the episode counters, bitwise.  The actions carry
-1, num_actions, INT32_MIN and INT32_MAX mixed in; the reference is handed them clamped on the host (cavoid.h: table actions are
clamped).  Every configuration asserts that what it is about happened: restarts, collisions, neighbours hidden by the clip or the
sensing horizon."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.cfg_regimes import TABLE5, TABLE32, WIDE          # (the tables live beside the other off-default cases)
from tests.gpu_support import F_PRESENT, INT32_MAX, INT32_MIN, _actions, _make_env, _Reference, _Subject

pytestmark = pytest.mark.gpu

# the form's switches; CAVOID_QUAD=0 everywhere: a one-step launch (K = 1) is env_kernel's plain step
FORMS = {"relay": dict(CAVOID_PIPELINE="2"), "pipe": dict(CAVOID_PIPELINE="1"), "loop_pf": dict(CAVOID_PIPELINE="0"),
         "loop": dict(CAVOID_PREFETCH_POOL="0")}
def _launch_lengths(N, lookahead=0):
    ring = 8 if N <= 5 else 4                               # relay_ring<N>() (cavoid_relay.hpp)
    lens = [1, 2, 3, 4, 5, 6, ring - 1, ring, ring + 1, 47, 48, 49, 63, 64, 65, 100, 129]
    if lookahead:                                           # a launch holds at most R - 1 steps with the look-ahead rings
        lens = [k for k in lens if k <= lookahead - 1]
    return lens


# id: (N, M, W, cavoid_cfg overrides, case options)
#   nc: consumers asked of the relay (None: the relay does not carry the configuration -- the PIPE form takes it);
#   nc_packed: what the relay really uses for packed records where the wider tile lowers it; env: CAVOID_* for every form's env;
#   expect: what must be seen to happen (restart, collision, clip, horizon, pressure)
NOT_RELAY = dict(nc=None)
CONFIGS = {
    # test_gpu_quad.py's CASES
    "n4-baseline-8192": (4, None, 8192, dict(), dict(nc=3)),
    "n4-scripted-ragged": (4, None, 1000, dict(gen_min_agents=2, gen_nonlearning_fraction=0.4), dict(nc=4)),
    "n4-generator-in-step": (4, None, 777, dict(gen_pool_size=0), dict(nc=2, forms=("loop",))),
    "n4-lookahead8": (4, None, 777, dict(gen_pool_size=0, gen_lookahead=8), dict(nc=2)),
    "n4-m2-clip": (4, 2, 600, dict(gen_min_agents=4), dict(nc=1, expect=("clip",))),
    "n4-closest-first": (4, None, 500, dict(sort_method="closest_first", gen_min_agents=3), dict(nc=2)),
    "n4-time-to-impact": (4, None, 500, dict(sort_method="time_to_impact", gen_min_agents=2), dict(nc=3)),
    "n4-u4-pipe-fallback": (4, None, 500, dict(done_agents_collide=0, gen_min_agents=2), NOT_RELAY),
    "n4-u7a-u7b": (4, None, 500, dict(sort_round_gap=0, sort_tie_lateral=0), dict(nc=4)),
    "n4-u2-slope": (4, None, 500, dict(wrap_closed_end=1, actions_fp32=1, close_penalty_slope=0.5), dict(nc=3)),
    "n4-max-turn": (4, None, 400, dict(dynamics="unicycle_max_turn_rate"), dict(nc=3)),
    "n4-max-turn-wide": (4, None, 400, dict(dynamics="unicycle_max_turn_rate", actions=WIDE), dict(nc=2)),
    "n3": (3, None, 1000, dict(gen_min_agents=1), dict(nc=2)),
    "n2": (2, None, 333, dict(), dict(nc=1)),
    "n5-nc4": (5, None, 400, dict(gen_min_agents=2, gen_nonlearning_fraction=0.2), dict(nc=4, nc_packed=3)),
    "n6": (6, None, 300, dict(gen_min_agents=2, gen_nonlearning_fraction=0.2), dict(nc=2)),
    "n10-pipe-fallback": (10, None, 257, dict(gen_min_agents=2, gen_nonlearning_fraction=0.2, gen_pool_size=300), NOT_RELAY),
    "n10-m3-clip": (10, 3, 200, dict(gen_min_agents=4, gen_pool_size=300), dict(nc=None, expect=("clip",))),
    # the relay's configuration space beyond them
    "n6-m2-clip": (6, 2, 300, dict(gen_min_agents=4), dict(nc=3, expect=("clip",))),
    "n4-u7a": (4, None, 500, dict(sort_round_gap=0), dict(nc=1)),
    "n4-u7b": (4, None, 500, dict(sort_tie_lateral=0), dict(nc=2)),
    "n4-u2": (4, None, 500, dict(wrap_closed_end=1), dict(nc=3)),
    "n5-u2-u7a-u7b": (5, None, 400, dict(wrap_closed_end=1, sort_round_gap=0, sort_tie_lateral=0, gen_min_agents=3), dict(nc=4, nc_packed=3)),
    "n4-actions-f64": (4, None, 500, dict(actions_fp32=0), dict(nc=3)),
    "n6-max-turn-closest-first": (6, None, 300, dict(dynamics="unicycle_max_turn_rate", actions=WIDE, sort_method="closest_first",
                                                     gen_min_agents=3), dict(nc=4)),
    "n4-evaluate-mode": (4, None, 500, dict(evaluate_mode=1, gen_min_agents=2, gen_nonlearning_fraction=0.3), dict(nc=2)),
    "n4-no-timeout": (4, None, 500, dict(timeout_enabled=0), dict(nc=3)),
    "n4-table5": (4, None, 500, dict(actions=TABLE5), dict(nc=3, straight=0)),
    "n4-table32": (4, None, 500, dict(actions=TABLE32), dict(nc=4, straight=16)),
    "n5-m2-horizon-step-reward": (5, 2, 400, dict(sensing_horizon=3.0, reward_time_step=-0.01, gen_min_agents=4),
                                  dict(nc=2, expect=("clip", "horizon"))),
    "n4-lookahead64": (4, None, 500, dict(gen_pool_size=0, gen_lookahead=64), dict(nc=3)),
    "n4-pool1": (4, None, 500, dict(gen_pool_size=1), dict(nc=2)),
    "n1": (1, None, 200, dict(), dict(nc=2, expect=("nocollision",))),
    "n4-wpw3": (4, None, 1000, dict(gen_min_agents=2), dict(nc=3, env=dict(CAVOID_WPW="3"))),
    # restart pressure: a time budget of one step -- every world of every tile restarts at every step, far more restarts within a
    # few steps than the relay's 8-deep restart-event queue (kRelayEvq) holds
    "n4-restart-every-step": (4, None, 512, dict(max_time_ratio=0.01), dict(nc=3, expect=("pressure", "nocollision"))),
    "n2-restart-every-step": (2, None, 300, dict(max_time_ratio=0.01, gen_pool_size=7), dict(nc=1, expect=("pressure", "nocollision"))),
}


def _forms_for(N, over, opt):
    """(form key, kind) -> expected (form, consumers)"""
    latency = over.get("gen_pool_size", 65536) > 0 or over.get("gen_lookahead", 0) > 0
    names = opt.get("forms") or (("relay", "pipe", "loop_pf", "loop") if latency else ("loop",))
    out = {}
    for f in names:
        for kind in ("slots", "packed", "last"):
            if f == "relay":
                nc = opt["nc"]
                want = ("PIPE", 0) if nc is None else ("RELAY", opt.get("nc_packed", nc) if kind == "packed" else nc)
            else:
                want = {"pipe": ("PIPE", 0), "loop_pf": ("LOOP_PF", 0), "loop": ("LOOP", 0)}[f]
            out[(f, kind)] = want
    return out


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_every_launch_form_equals_the_plain_step(cid, monkeypatch):
    N, M, W, over, opt = CONFIGS[cid]
    seed = 41
    Mv = N - 1 if M is None else M
    lens = _launch_lengths(N, over.get("gen_lookahead", 0))
    kmax = max(lens)
    ref_env = _make_env(monkeypatch, W, N, M, seed, {}, over)
    ref = _Reference(ref_env, kmax)
    subjects = []
    for (f, kind), want in _forms_for(N, over, opt).items():
        ev = dict(FORMS[f], **opt.get("env", {}))
        if f == "relay" and opt["nc"] is not None:
            ev["CAVOID_RELAY_CONSUMERS"] = str(opt["nc"])
        subjects.append(_Subject(_make_env(monkeypatch, W, N, M, seed, ev, over), f, kind, want, kmax))
    ref_env.reset()
    for s in subjects:
        s.env.reset()
    rng = np.random.default_rng(7)
    A = int(ref_env.num_actions)
    total = 0
    seen_clip = seen_horizon = False
    for K in lens:
        raw, clamped = _actions(rng, K, W, N, A, opt.get("straight", 2))
        raw_d, cl_d = torch.from_numpy(raw).cuda(), torch.from_numpy(clamped).cuda()
        ref.run(cl_d)
        for s in subjects:
            s.launch(raw_d)
        total += K
        for s in subjects:
            s.check(ref, K, (cid, s.form, s.kind, "K=%d" % K, "after %d steps" % total))
        # per launch: the last step's observation -- neighbours hidden by the clip / the horizon
        fl = ref_env.get_state()[2].view(W, N)
        rows = (fl & F_PRESENT) != 0
        present = rows.sum(dim=1, keepdim=True)
        seen = ref.obs[K - 1][..., 1]
        seen_clip |= bool(((present - 1 > Mv) & rows).any().item())
        seen_horizon |= bool(((seen < torch.clamp(present - 1, max=Mv).float()) & rows).any().item())
    expect = opt.get("expect", ())
    ep = ref_env.episode
    assert ep.max().item() >= 1, "no world restarted"
    if "pressure" in expect:
        assert ep.min().item() >= total // 2, ("every world restarts about every step", ep.min().item(), total)
    if "nocollision" not in expect:
        assert ref.coll.item(), "no collision in the run"
    if "clip" in expect:
        assert seen_clip, "no world with more neighbours than the observation has slots"
    if "horizon" in expect:
        assert seen_horizon, "the sensing horizon hid no neighbour"
    for s in subjects:
        s.env.close()
    ref_env.close()


@pytest.mark.parametrize("N,W,form", [(4, 300, "relay"), (4, 300, "pipe"), (4, 300, "loop_pf"), (4, 300, "loop"), (6, 200, "relay"),
                                      (3, 500, "relay")])
def test_padded_and_zero_action_strides(N, W, form, monkeypatch):
    """cavoid_step_autoreset_n through ctypes with a discrete action_stride beyond W*N (a padded buffer: step t reads the slice at
    t * stride) and with action_stride = 0 (every step reads the same slice), out-of-range actions in both."""
    from rl_collision_avoidance_amd import _lib
    seed, A = 13, 11
    ref_env = _make_env(monkeypatch, W, N, None, seed, {}, {})
    ev = dict(FORMS[form])
    if form == "relay":
        ev["CAVOID_RELAY_CONSUMERS"] = "2"
    env = _make_env(monkeypatch, W, N, None, seed, ev, {})
    expect = {"relay": ("RELAY", 2), "pipe": ("PIPE", 0), "loop_pf": ("LOOP_PF", 0), "loop": ("LOOP", 0)}[form]
    ref = _Reference(ref_env, 129)
    sub = _Subject(env, form, "slots", expect, 129)
    slots = sub.slots
    ref_env.reset(); env.reset()
    lib = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    rng = np.random.default_rng(3)
    pad = 37
    for K, zero in ((9, False), (65, False), (3, True), (129, False), (66, True), (2, False)):
        raw, clamped = _actions(rng, K, W, N, A, 2)
        if zero:                                           # one slice for every step
            raw[:], clamped[:] = raw[0], clamped[0]
            buf, stride = torch.from_numpy(raw[0].ravel().copy()).cuda(), 0
        else:                                              # step t at t * (W*N + pad): the padding holds garbage the kernel must not read
            host = rng.integers(INT32_MIN, INT32_MAX, size=(K, W * N + pad), dtype=np.int64).astype(np.int32)
            host[:, :W * N] = raw.reshape(K, W * N)
            buf, stride = torch.from_numpy(host).cuda(), W * N + pad
        rc = lib.cavoid_step_autoreset_n(env._h, p(buf), stride, K, W, p(slots.obs), p(slots.rewards), p(slots.done),
                                         p(slots.game_over), None)
        assert rc == 0, rc
        ref.run(torch.from_numpy(clamped).cuda())
        sub.check(ref, K, (form, K, "stride 0" if zero else "padded"))
    assert ref_env.episode.max().item() >= 1
    torch.cuda.synchronize()
    env.close(); ref_env.close()
