"""env_relay_kernel with two tiles per workgroup (CAVOID_RELAY_TILES=2: one workgroup of up to 16 wavefronts owns the tiles 2 b and
2 b + 1, csrc/cavoid_relay.hpp) against the plain one-step kernel and against one tile per workgroup (CAVOID_RELAY_TILES=1), BITWISE:
observations, rewards, done flags, game_over of every step, the state and the episode counters after every launch.

The reference is taken the way tests/test_gpu_launch_forms.py takes it (its helpers are used as they are): one env steps one launch
per step with the host-clamped actions.  Every launch asserts the form that ran, the consumer count it really used and -- through
cavoid_relay_last_tiles -- that the workgroups really held two tiles.

Shapes: one tile without a partner (16 worlds at 16 worlds per tile), a partner of one world (17), an odd tile count (33), 48, 300 and,
once, 8192 worlds at N = 4; 70 worlds at N = 2, 3, 5.  Launch lengths 1, 2, 3, 9 (the 8-slot rings wrap), 20 and 65 (the action ring
wraps); per-step slots, packed records, last-step-only outputs; 2, 3 and 4 consumers, asked for explicitly."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.gpu_support import ONE_STEP, _actions, _lookahead_env as _env, _make_env, _Reference, _same_bits as _same, _same_slots, _same_state, _Subject

pytestmark = pytest.mark.gpu

LENS = (1, 2, 3, 9, 20, 65)
KINDS = ("slots", "packed", "last")


def _last_tiles():
    from rl_collision_avoidance_amd import _lib
    f = _lib.lib().cavoid_relay_last_tiles
    f.restype, f.argtypes = C.c_int32, []
    return f()


def _relay_env(monkeypatch, W, N, seed, tiles, nc, over):
    ev = dict(CAVOID_PIPELINE="2", CAVOID_RELAY_TILES=str(tiles))
    if nc is not None:
        ev["CAVOID_RELAY_CONSUMERS"] = str(nc)
    try:
        return _make_env(monkeypatch, W, N, None, seed, ev, over)
    finally:
        monkeypatch.delenv("CAVOID_RELAY_TILES", raising=False)


class _Pair(object):
    """the same output kind through two tiles per workgroup and through one"""

    def __init__(self, monkeypatch, W, N, seed, nc, over, kind, kmax):
        self.duo = _Subject(_relay_env(monkeypatch, W, N, seed, 2, nc, over), "relay-duo", kind, None, kmax)
        self.solo = _Subject(_relay_env(monkeypatch, W, N, seed, 1, nc, over), "relay-solo", kind, None, kmax)
        self.kind = kind

    def launch_and_check(self, raw, ref, K, nc, tag):
        used = {}
        for sub, tiles in ((self.solo, 1), (self.duo, 2)):
            sub.launch(raw)
            form, used[tiles] = sub.env.last_step_form
            if K == 1:                                      # a one-step launch is env_kernel's plain step, whatever the knobs say
                assert (form, used[tiles]) == ("STEP", 0), (tag, tiles)
            else:
                assert form == "RELAY" and _last_tiles() == tiles, (tag, tiles, form, _last_tiles())
            sub.expect = (form, used[tiles])
            sub.check(ref, K, tag + (sub.form,))
        # the consumer count: what was asked for, unless the packed records' wider tile lowers it -- then for both forms alike
        assert used[1] == used[2], (tag, used)
        if K > 1 and self.kind != "packed":
            assert used[2] == nc, (tag, used)
        if K > 1:
            assert 2 <= used[2] <= nc, (tag, used)
        d, s = self.duo, self.solo                          # ... and the two forms against each other, directly
        if self.kind == "slots":
            for n in ("obs", "rewards", "done", "game_over"):
                _same(getattr(d.slots, n)[:K], getattr(s.slots, n)[:K], tag + ("duo vs solo", n))
        elif self.kind == "packed":
            _same(d.slots.packed[:K], s.slots.packed[:K], tag + ("duo vs solo", "packed"))
            _same(d.slots.game_over[:K], s.slots.game_over[:K], tag + ("duo vs solo", "game_over"))
        else:
            for n in ("obs", "rewards", "done", "game_over"):
                _same(getattr(d.env, n), getattr(s.env, n), tag + ("duo vs solo", n))
        for x, y in zip(d.env.get_state(), s.env.get_state()):
            _same(x, y, tag + ("duo vs solo", "state"))
        _same(d.env.episode, s.env.episode, tag + ("duo vs solo", "episode"))

    def close(self):
        self.duo.env.close(); self.solo.env.close()


# id: (N, W, consumers asked for, launch lengths, output kinds, cavoid_cfg overrides)
CASES = {
    "n4-w16-no-partner": (4, 16, 2, LENS, KINDS, dict(gen_pool_size=300)),
    "n4-w17-partner-of-one-world": (4, 17, 3, LENS, KINDS, dict(gen_pool_size=300, gen_min_agents=2, gen_nonlearning_fraction=0.3)),
    "n4-w33-three-tiles": (4, 33, 4, LENS, KINDS, dict(gen_pool_size=7)),
    "n4-w48": (4, 48, 2, LENS, KINDS, dict(gen_pool_size=300, max_time_ratio=0.3)),
    "n4-w300": (4, 300, 4, LENS, KINDS, dict(gen_min_agents=2)),
    "n4-w300-three-consumers": (4, 300, 3, (9, 20), ("slots",), dict()),
    "n4-w8192": (4, 8192, 4, (20,), ("slots",), dict()),
    "n2-w70": (2, 70, 3, LENS, KINDS, dict(gen_pool_size=64)),
    "n3-w70": (3, 70, 4, LENS, KINDS, dict(gen_min_agents=1)),
    "n5-w70": (5, 70, 4, LENS, KINDS, dict(gen_min_agents=2, gen_nonlearning_fraction=0.2)),
}


@pytest.mark.parametrize("cid", list(CASES))
def test_two_tiles_per_workgroup_equal_the_plain_step_and_one_tile_per_workgroup(cid, monkeypatch):
    N, W, nc, lens, kinds, over = CASES[cid]
    seed, kmax = 43, max(lens)
    ref_env = _make_env(monkeypatch, W, N, None, seed, {}, over)
    ref = _Reference(ref_env, kmax)
    pairs = [_Pair(monkeypatch, W, N, seed, nc, over, kind, kmax) for kind in kinds]
    ref_env.reset()
    for p in pairs:
        p.duo.env.reset(); p.solo.env.reset()
    rng = np.random.default_rng(11)
    A = int(ref_env.num_actions)
    total = 0
    for K in lens:
        raw, clamped = _actions(rng, K, W, N, A, 2)
        ref.run(torch.from_numpy(clamped).cuda())
        total += K
        raw_d = torch.from_numpy(raw).cuda()
        for p in pairs:
            p.launch_and_check(raw_d, ref, K, nc, (cid, p.kind, "K=%d" % K, "after %d steps" % total))
    if "max_time_ratio" in over:                            # (the short time budget: worlds restart inside the launches)
        assert ref_env.episode.min().item() >= 1, "a world never restarted"
    for p in pairs:
        p.close()
    ref_env.close()


def test_restarts_and_new_collisions_in_both_tiles_of_a_workgroup_in_one_launch(monkeypatch):
    """Pressure: a short time budget (worlds restart every few steps) in a small arena (GEN v2 boxes of 2 m half side for four agents,
    scenarios from a pool: paths cross at once), 64 worlds = two workgroups of two tiles.  In one and the same launch a tile with an even
    index and the odd tile of the SAME workgroup must each see a restart and a new collision: the surprise path (D's re-post, the event
    queue, the loader's refill) of both tiles at work side by side."""
    N, W, K, nc, seed = 4, 64, 20, 4, 17
    over = dict(gen_mode=1, gen_pool_size=300, gen_box_small=(2.0, 2.0), gen_box_large=(2.0, 2.0), gen_min_trip=1.5, gen_min_agents=4,
                max_time_ratio=0.5)
    wpt = 64 // N
    ref_env = _make_env(monkeypatch, W, N, None, seed, {}, over)
    ref = _Reference(ref_env, K)
    pair = _Pair(monkeypatch, W, N, seed, nc, over, "slots", K)
    ref_env.reset(); pair.duo.env.reset(); pair.solo.env.reset()
    rng = np.random.default_rng(5)
    A = int(ref_env.num_actions)
    both = 0
    for launch in range(4):
        raw, clamped = _actions(rng, K, W, N, A, 2, p_edge=0.0)
        ref.run(torch.from_numpy(clamped).cuda())
        pair.launch_and_check(torch.from_numpy(raw).cuda(), ref, K, nc, ("pressure", "launch %d" % launch))
        restart = ref.go[:K].bool().any(dim=0).view(W // wpt, wpt).any(dim=1).cpu().numpy()          # per tile
        # a NEW collision pays the collision reward at its step (the step that ends the world included)
        hit = (ref.rew[:K] <= ref.r_coll).any(dim=0).view(W // wpt, wpt * N).any(dim=1).cpu().numpy()
        busy = restart & hit
        print("launch %d: tiles with a restart %s, with a new collision %s" % (launch, restart.astype(int), hit.astype(int)))
        both += int(any(busy[2 * b] and busy[2 * b + 1] for b in range(len(busy) // 2)))
    assert both >= 1, "no launch with a restart and a new collision in both tiles of one workgroup"
    pair.close(); ref_env.close()


@pytest.mark.parametrize("W", [40, 64])
def test_lookahead_rings_with_the_top_up_in_both_tiles(W, monkeypatch):
    """Look-ahead rings topped up inside the launch by the T wavefronts of both tiles (16 wavefronts per workgroup at four consumers):
    six consecutive launches of K = R / 2 steps with every world restarting at every step, held bitwise to generation inside the step as
    tests/test_gpu_lookahead_topup.py does -- the rings wrap three times; a slot one T left stale or wrote for the wrong tile shows as a
    wrong scenario.  Not one refill launch follows the first fill.  W = 40: an odd tile count, the last workgroup has one tile."""
    N, K, R, launches, seed = 4, 8, 16, 6, 11
    monkeypatch.setenv("CAVOID_RELAY_TILES", "2")
    monkeypatch.setenv("CAVOID_RELAY_CONSUMERS", "4")
    a, b = _env(W, N, seed, 0, **ONE_STEP), _env(W, N, seed, R, **ONE_STEP)
    monkeypatch.delenv("CAVOID_RELAY_TILES"); monkeypatch.delenv("CAVOID_RELAY_CONSUMERS")
    assert torch.equal(a.reset(), b.reset()) and _same_state(a, b)
    primed = b.lookahead_info[0]
    g = torch.Generator(device="cuda").manual_seed(seed)
    sa, sb = a.new_step_slots(K), b.new_step_slots(K)
    for l in range(launches):
        acts = torch.randint(0, 11, (K, W, N), generator=g, device="cuda", dtype=torch.int32)
        a.step_autoreset_n(acts, K, slots=sa)
        b.step_autoreset_n(acts, K, slots=sb)
        assert b.last_step_form == ("RELAY", 4) and _last_tiles() == 2, (l, b.last_step_form, _last_tiles())
        assert _same_slots(sa, sb, K), l
        assert _same_state(a, b), l
    assert primed == 1 and b.lookahead_info[0] == primed                     # every launch carried its top-up
    assert (b.episode.cpu().numpy().view(np.uint32) == launches * K).all()
    a.close(); b.close()
