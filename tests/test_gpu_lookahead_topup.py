"""The relay launch tops up its own look-ahead rings (`env_relay_kernel`'s top-up wavefront, csrc/cavoid_relay.hpp): with GEN v1
scenarios and launches of at most R / 2 steps no `ahead_fill_kernel` launch sits in front of a relay launch any more.  Everything here
is held BITWISE -- obs, rewards, done, game_over of every step, state and episodes -- to the same run with `gen_lookahead = 0,
gen_pool_size = 0` (generation inside the step), as tests/test_gpu_lookahead.py does, and the refill launches are counted
(`cavoid_ahead_info`): the first fill stays, the forms without the role (one-step launches, resets, N = 6, GEN v2, anything captured
into a hipGraph) keep theirs."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.gpu_support import ONE_STEP, _lookahead_env as _env, _same_slots, _same_state

pytestmark = pytest.mark.gpu

# the short episodes of test_gpu_lookahead.py::test_random_launch_sequences_keep_the_rings_covered (restarts every few steps, not all at once)
SHORT = dict(max_time_ratio=0.3)


def _relay_launches(W, N, K, R, launches, over, seed=11):
    """`launches` K-step launches on rings of R episodes against generation inside the step; returns (refill launches right after the
    first fill, refill launches at the end, episodes of the look-ahead env)"""
    a, b = _env(W, N, seed, 0, **over), _env(W, N, seed, R, **over)
    assert torch.equal(a.reset(), b.reset()) and _same_state(a, b)
    primed = b.lookahead_info[0]
    g = torch.Generator(device="cuda").manual_seed(seed)
    sa, sb = a.new_step_slots(K), b.new_step_slots(K)
    for l in range(launches):
        acts = torch.randint(0, 11, (K, W, N), generator=g, device="cuda", dtype=torch.int32)
        a.step_autoreset_n(acts, K, slots=sa)
        b.step_autoreset_n(acts, K, slots=sb)
        assert b.last_step_form[0] == "RELAY", (l, b.last_step_form)
        assert _same_slots(sa, sb, K), l
        assert _same_state(a, b), l
    out = primed, b.lookahead_info[0], b.episode.cpu().numpy().view(np.uint32).copy()
    a.close(); b.close()
    return out


@pytest.mark.parametrize("over", [ONE_STEP, SHORT], ids=["one_step_episodes", "short_episodes"])
def test_ring_boundary_r_equals_two_launches(over):
    """R = 2 K exactly, a ragged last tile (W = 40 at 16 worlds per tile), 40 launches back to back: the rings wrap twenty times when
    every world restarts at every step, and not one refill launch follows the first fill"""
    K, R, launches = 8, 16, 40
    primed, refills, episodes = _relay_launches(40, 4, K, R, launches, over)
    assert primed == 1 and refills == primed
    if over is ONE_STEP:                                                     # the reset started episode 0; every step since started another
        assert (episodes == launches * K).all()
    else:
        assert episodes.min() >= 1


@pytest.mark.parametrize("N,W", [(2, 33), (5, 33), (4, 1)])
def test_other_agent_counts_and_a_single_world(N, W):
    K, R, launches = 8, 16, 12
    primed, refills, episodes = _relay_launches(W, N, K, R, launches, ONE_STEP)
    assert primed == 1 and refills == primed
    assert (episodes == launches * K).all()


def test_mixed_sequences_keep_the_other_forms_refills():
    """relay launches of random length (up to R / 4) with, between two of them, a short burst of one-step launches, a masked reset or --
    behind a burst longer than the ring -- a re-seeding.  The sequence is built so that the budget a relay launch finds is always enough
    (at least R - 8 after a relay launch, at most 6 taken by what lies between two of them, and a re-seed primes afresh): a relay call
    never launches a refill; the one-step launches and the resets launch theirs exactly when their budget is short of 2, as before."""
    W, N, R, seed = 70, 4, 32, 5
    rng = np.random.default_rng(seed)
    a, b = _env(W, N, seed, 0, **SHORT), _env(W, N, seed, R, **SHORT)
    assert torch.equal(a.reset(), b.reset())
    g = torch.Generator(device="cuda").manual_seed(seed)
    sa, sb = a.new_step_slots(8), b.new_step_slots(8)
    primings, at_single, relays = 1, 0, 0
    assert b.lookahead_info[0] == primings

    def single(it):
        nonlocal at_single
        before, budget = b.lookahead_info
        acts = torch.randint(0, 11, (W, N), generator=g, device="cuda", dtype=torch.int32)
        ra, rb = a.step_autoreset(acts), b.step_autoreset(acts)
        assert all(torch.equal(x, y) for x, y in zip(ra, rb)), (it, "single")
        grew = b.lookahead_info[0] - before
        assert grew == (1 if budget < 2 else 0), (it, budget, grew)
        at_single += grew

    after_relay = False
    for it in range(40):
        kind = rng.random() if after_relay else 0.0                          # (something else only BETWEEN two relay launches)
        after_relay = kind < 0.5
        if kind < 0.5:
            K = int(rng.integers(2, 9))
            before, budget = b.lookahead_info
            assert budget >= K, (it, budget, K)                              # (how the sequence is built, see above)
            acts = torch.randint(0, 11, (K, W, N), generator=g, device="cuda", dtype=torch.int32)
            a.step_autoreset_n(acts, K, slots=sa)
            b.step_autoreset_n(acts, K, slots=sb)
            assert b.last_step_form[0] == "RELAY" and _same_slots(sa, sb, K), (it, K)
            assert b.lookahead_info == (before, R - K), (it, K)
            relays += 1
        elif kind < 0.75:
            for _ in range(int(rng.integers(1, 7))):
                single(it)
        elif kind < 0.87:
            before, budget = b.lookahead_info
            mask = (torch.rand(W, generator=g, device="cuda") < 0.4).to(torch.uint8)
            assert torch.equal(a.reset(mask), b.reset(mask)), (it, "reset")
            assert b.lookahead_info[0] - before == (1 if budget < 2 else 0), (it, "reset")
            at_single += b.lookahead_info[0] - before
        else:
            for _ in range(R + 3):                                           # longer than the ring: the one-step form must refill
                single(it)
            s2 = int(rng.integers(0, 1 << 30))
            a.seed(s2); b.seed(s2)
            before = b.lookahead_info[0]
            assert torch.equal(a.reset(), b.reset()), (it, "reseed")
            assert b.lookahead_info[0] == before + 1                         # the first fill for the new seed
            primings += 1
        assert _same_state(a, b), it
    assert relays >= 10 and primings >= 2 and at_single >= 1
    assert b.lookahead_info[0] == primings + at_single
    a.close(); b.close()


@pytest.mark.parametrize("N,over", [(6, ONE_STEP), (4, dict(gen_mode=1, **ONE_STEP))], ids=["six_agents", "gen_v2"])
def test_forms_without_the_role_keep_the_refill_launch(N, over):
    """N = 6 (its registers leave no room for a seventh wavefront at two workgroups per CU) and GEN v2 (wave-cooperative rejection
    sampling) still run the relay kernel behind refill launches: after the first launch every launch of K = R / 2 steps needs one"""
    K, R, launches = 8, 16, 8
    primed, refills, episodes = _relay_launches(33, N, K, R, launches, over)
    assert primed == 1 and refills == primed + launches - 1
    assert (episodes == launches * K).all()


def test_a_captured_relay_sequence_keeps_the_refill_launch():
    """a relay launch captured into a hipGraph carries its refill (host bookkeeping cannot follow the replays), and once the graph exists
    the eager launches do too"""
    W, N, K, R, seed = 40, 4, 8, 16, 23
    a, b = _env(W, N, seed, 0, **ONE_STEP), _env(W, N, seed, R, **ONE_STEP)
    assert torch.equal(a.reset(), b.reset())
    g = torch.Generator(device="cuda").manual_seed(seed)
    sa, sb = a.new_step_slots(K), b.new_step_slots(K)
    buf = torch.zeros((K, W, N), device="cuda", dtype=torch.int32)

    def acts():
        buf.copy_(torch.randint(0, 11, (K, W, N), generator=g, device="cuda", dtype=torch.int32))
        return buf

    a.step_autoreset_n(acts(), K, slots=sa)
    b.step_autoreset_n(buf, K, slots=sb)                                     # eager, with the top-up wavefront
    assert b.lookahead_info[0] == 1 and _same_slots(sa, sb, K)
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            b.step_autoreset_n(buf, K, slots=sb)
    torch.cuda.synchronize()
    assert b.last_step_form[0] == "RELAY" and b.lookahead_info[0] == 2       # the captured refill
    for r in range(4):
        a.step_autoreset_n(acts(), K, slots=sa)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_slots(sa, sb, K) and _same_state(a, b), r
    before = b.lookahead_info[0]
    for r in range(3):
        a.step_autoreset_n(acts(), K, slots=sa)
        b.step_autoreset_n(buf, K, slots=sb)
        assert b.last_step_form[0] == "RELAY" and _same_slots(sa, sb, K) and _same_state(a, b), r
    assert b.lookahead_info[0] == before + 3
    assert (b.episode.cpu().numpy().view(np.uint32) == 8 * K).all()
    a.close(); b.close()
