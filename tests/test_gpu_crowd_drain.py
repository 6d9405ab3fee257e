"""The hand-over to the trainer (cavoid_rollout_compact: BatchedRollout.drain / drain_begin / drain_end) on rows wider than 255 floats:
crowd worlds of 37 agents (D = 257, the first width the copy loop's e / D limit used to refuse), of 64 agents (D = 446) and an env of 8
agents padded to 64 observed (D = 453, the widest row the env makes).  Every drained row is held bit for bit to the experience ring it was
copied from."""
import pytest

torch = pytest.importorskip("torch")

from tests.gpu_support import _env

pytestmark = pytest.mark.gpu


def _rollout(N, M=None, seed=2, steps=12):
    """64 worlds acting on the fused crowd policy, cleaned mode (the training CLI's), `steps` steps in"""
    from rl_collision_avoidance_amd.ga3c.network import NetworkVP_rnn
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    env = _env(64, N, M, seed=seed, gen_pool_size=0, gen_min_agents=2)
    pol = FusedPolicy(NetworkVP_rnn(env.config).to("cuda:0"), seed=3)
    assert pol.crowd
    roll = BatchedRollout(env, pol, time_max=3, reflush_done=False)
    roll.reset()
    for _ in range(steps):
        roll.step()
    return env, roll


def _snapshot(roll):
    return roll.x.clone(), roll.ret.clone(), roll.act_ring.clone(), roll.emit_t.clone()


def _assert_rows_are_the_rings(batch, snap, roll, N, lo, hi):
    x, ret, act, emit = snap
    blocks = torch.tensor([s % roll.ring_len for s in range(lo, hi)], dtype=torch.long, device=x.device)
    assert len(batch) == int((emit[blocks] >= 0).sum()) and len(batch) > 0
    assert batch.dropped == 0
    src = batch.src.long()
    assert int(src[:, 2].min()) >= lo and int(src[:, 2].max()) < hi
    block, slot = src[:, 2] % roll.ring_len, src[:, 0] * N + src[:, 1]
    assert torch.equal(batch.x, x[block, slot])
    assert torch.equal(batch.r, ret[block, slot])
    assert torch.equal(batch.a_index, act[block, slot].to(torch.int32))
    assert torch.equal(src[:, 3], emit[block, slot].long())
    key = src[:, 2] * roll.slots + slot
    assert key.unique().numel() == key.numel()              # no row twice


@pytest.mark.parametrize("N,M,D", [(37, None, 257), (64, None, 446), (8, 64, 453)])
def test_wide_rows_drain_bit_for_bit(N, M, D):
    env, roll = _rollout(N, M)
    assert env.obs_width - 1 == D
    snap = _snapshot(roll)
    lo, hi = roll.drained_until, roll.step_index - roll.margin
    assert hi - lo == 7
    batch = roll.drain(provenance=True)
    assert batch.x.shape[1] == D and roll.drained_until == hi
    _assert_rows_are_the_rings(batch, snap, roll, N, lo, hi)
    assert all(torch.equal(a, b) for a, b in zip(snap, _snapshot(roll)))     # (a plain drain leaves the ring as it was)
    roll.close(); env.close()


def test_wide_rows_pipelined_hand_over_equals_drain():
    """drain_begin / drain_end deliver the rows drain() delivers, at 64 agents per world (tests/test_gpu_actor.py holds the same at 4)"""
    import numpy as np
    env_a, a = _rollout(64, steps=0)
    env_b, b = _rollout(64, steps=0)
    rows_a, rows_b, pending = [], [], None
    for _ in range(4):
        for _ in range(4):
            a.step()
            b.step()
        rows_a.append(a.drain(provenance=True))
        h = b.drain_begin(provenance=True)
        if pending is not None:
            rows_b.append(b.drain_end(pending))
        pending = h
    rows_b.append(b.drain_end(pending))
    assert a.frames == b.frames > 0
    sa = torch.cat([r.src for r in rows_a]).cpu().numpy()
    sb = torch.cat([r.src for r in rows_b]).cpu().numpy()
    for name in ("x", "r", "a_index", "src"):
        xa = torch.cat([getattr(r, name) for r in rows_a]).cpu().numpy()
        xb = torch.cat([getattr(r, name) for r in rows_b]).cpu().numpy()
        assert np.array_equal(xa[np.lexsort(sa.T[::-1])], xb[np.lexsort(sb.T[::-1])]), name
    for r in (a, b):
        r.close()
    env_a.close(); env_b.close()


def test_wide_rows_flush_all_hands_every_row_out_once():
    N = 64
    env, roll = _rollout(N)
    snap = _snapshot(roll)
    first = roll.drain(flush_all=True, provenance=True)
    _assert_rows_are_the_rings(first, snap, roll, N, 0, roll.step_index)
    assert int((roll.emit_t >= 0).sum()) == 0               # every handed-out row is stamped
    again = roll.drain(flush_all=True, provenance=True)
    assert len(again) == 0 and again.dropped == 0
    for _ in range(4):
        roll.step()
    later = roll.drain(flush_all=True, provenance=True)
    assert len(later) > 0 and torch.isfinite(later.x).all()
    key = lambda b: set((b.src[:, 2].long() * roll.slots + b.src[:, 0].long() * N + b.src[:, 1].long()).tolist())
    assert not (key(first) & key(later))
    roll.close(); env.close()
