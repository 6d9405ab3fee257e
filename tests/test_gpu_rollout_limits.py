"""``cavoid_rollout_push`` / ``cavoid_rollout_compact`` at the limits of what the C ABI accepts, on SCRIPTED input (tests/rollout_scripts.py:
the host test tests/test_rollout_scripts.py holds that every script reaches every flush kind) against oracle/rollout_oracle.py:
time_max 1, 2, 31 (all 32 registers of the backward pass live), 32, 33, 40 and 254 (the serial pass), the smallest ring the entry point
accepts, the device-side step counter, and the three capacity paths -- a full duplicate buffer, a full episode log, a compaction without
room.  Raw binding, caller-owned tensors, the way ``BatchedRollout`` calls it.  Every output tensor carries GUARD rows of a canary
pattern behind the capacity the library is given; no test depends on what an out-of-bounds write would do."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import rollout_scripts as rs

pytestmark = pytest.mark.gpu

GUARD = 64
CANARY_F, CANARY_I = -12345.5, -777


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(rows, width, dtype):
    """[rows + GUARD, width] (or [rows + GUARD]) of the canary pattern: the library is told ``rows``"""
    shape = (rows + GUARD, width) if width else (rows + GUARD,)
    return torch.full(shape, CANARY_F if dtype.is_floating_point else CANARY_I, dtype=dtype, device="cuda")


def _intact(t, rows):
    want = CANARY_F if t.dtype.is_floating_point else CANARY_I
    return bool((t[rows:] == want).all().item())


class Store(object):
    """A caller-owned experience store over one timeline's inputs."""

    def __init__(self, case, ring_len, dup_capacity=None, ep_capacity=None):
        from rl_collision_avoidance_amd import _lib
        self._lib, self._check = _lib.lib(), _lib.check
        tl = self.tl = rs.case_timeline(case)
        self.case, self.RL, self.S, self.D = case, int(ring_len), case.W * case.N, case.D
        dev = "cuda"
        self.inputs = [torch.from_numpy(v).to(dev) for v in (tl.prev_obs, tl.actions, tl.values, tl.rewards, tl.done, tl.game_over)]
        RL, S, D = self.RL, self.S, self.D
        self.x = torch.zeros((RL, S, D), dtype=torch.float32, device=dev)
        self.val = torch.zeros((RL, S), dtype=torch.float64, device=dev)
        self.ret = torch.zeros((RL, S), dtype=torch.float32, device=dev)
        self.act = torch.zeros((RL, S), dtype=torch.uint8, device=dev)
        self.emit_t = torch.full((RL, S), -1, dtype=torch.int32, device=dev)
        self.dup_capacity = int(dup_capacity if dup_capacity is not None else tl.T * S)
        self.ep_capacity = int(ep_capacity if ep_capacity is not None else tl.T * case.W)
        self.dup_x = _guarded(self.dup_capacity, D, torch.float32)
        self.dup_r = _guarded(self.dup_capacity, 0, torch.float32)
        self.dup_a = _guarded(self.dup_capacity, 0, torch.int32)
        self.dup_src = _guarded(self.dup_capacity, 4, torch.int32)
        self.dup_count = torch.zeros((2,), dtype=torch.int32, device=dev)
        self.ep_out = _guarded(self.ep_capacity, 3, torch.float32)
        self.ep_count = torch.zeros((2,), dtype=torch.int32, device=dev)
        self.counts = torch.zeros((2,), dtype=torch.int32, device=dev)
        h = C.c_void_p()
        self._check(self._lib.cavoid_rollout_create(case.W, case.N, 1 + D, case.time_max, case.discount, case.reflush, RL, 0, C.byref(h)),
                    "cavoid_rollout_create")
        self._h = h

    def close(self):
        torch.cuda.synchronize()
        self._lib.cavoid_rollout_destroy(self._h)
        self._h = None

    def push(self, t, step):
        obs, actions, values, rewards, done, game_over = (v[t] for v in self.inputs)
        self._check(self._lib.cavoid_rollout_push(
            self._h, _p(obs), _p(actions), _p(values), _p(rewards), _p(done), _p(game_over), step,
            _p(self.x), _p(self.val), _p(self.ret), _p(self.act), _p(self.emit_t),
            _p(self.dup_x), _p(self.dup_r), _p(self.dup_a), _p(self.dup_src), _p(self.dup_count), self.dup_capacity,
            _p(self.ep_out), _p(self.ep_count), self.ep_capacity, _stream()), "cavoid_rollout_push")

    def new_out(self, capacity):
        return (_guarded(capacity, self.D, torch.float32), _guarded(capacity, 0, torch.float32), _guarded(capacity, 0, torch.int32),
                _guarded(capacity, 4, torch.int32))

    def compact(self, lo, hi, mark_taken, out, at, capacity):
        """rows of the blocks [lo, hi) into ``out`` from row ``at`` on, ``capacity`` rows of room; returns (offered, dropped)"""
        ox, orr, oa, osrc = out
        assert 0 <= capacity and at + capacity + GUARD <= len(orr)           # the library's room ends GUARD rows before the tensors do
        self._check(self._lib.cavoid_rollout_compact(self._h, lo, hi, mark_taken, _p(self.x), _p(self.ret), _p(self.act), _p(self.emit_t),
                                                      _p(ox[at:]), _p(orr[at:]), _p(oa[at:]), _p(osrc[at:]), _p(self.counts), capacity,
                                                      _stream()), "cavoid_rollout_compact")
        offered, dropped = self.counts.tolist()
        return offered, dropped

    def duplicates(self):
        """the duplicate buffer's stored rows; asserts its counters' arithmetic and the guard rows"""
        offered, dropped = self.dup_count.tolist()
        n = min(offered, self.dup_capacity)
        assert dropped == offered - n
        assert all(_intact(t, self.dup_capacity) for t in (self.dup_x, self.dup_r, self.dup_a, self.dup_src)), "a write behind dup_capacity"
        return rs.Rows(*(t[:n].cpu().numpy() for t in (self.dup_x, self.dup_r, self.dup_a, self.dup_src))), offered, dropped

    def episodes(self):
        offered, dropped = self.ep_count.tolist()
        n = min(offered, self.ep_capacity)
        assert dropped == offered - n
        assert _intact(self.ep_out, self.ep_capacity), "a write behind ep_capacity"
        return self.ep_out[:n].cpu().numpy(), offered, dropped


def _rows(out, n):
    return rs.Rows(*(t[:n].cpu().numpy() for t in out))


def _cat(*parts):
    return rs.Rows(*(np.concatenate([np.asarray(p[k]) for p in parts]) for k in range(4)))


def _run_smallest_ring(case, device_counter=False):
    """ring_len = time_max + 2, the smallest the entry point accepts: after the push of step t the block of step t - time_max - 1 --
    final by the header's rule for one step, overwritten by the next push -- is compacted (mark_taken = 0), and after the last push
    the blocks that are still alive.  A row emitted later than the header promises goes missing.  Returns (store, ring rows)."""
    tl, tm = rs.case_timeline(case), case.time_max
    st = Store(case, ring_len=tm + 2)
    total = tl.T * st.S
    out = st.new_out(total)
    n = 0
    for t in range(tl.T):
        st.push(t, -1 if device_counter else t)
        s = t - tm - 1
        if s >= 0:
            offered, dropped = st.compact(s, s + 1, 0, out, n, total - n)
            assert dropped == 0 and offered <= st.S
            n += offered
    offered, dropped = st.compact(tl.T - tm - 1, tl.T, 0, out, n, total - n)
    assert dropped == 0
    n += offered
    assert all(_intact(t, total) for t in out)
    return st, _rows(out, n)


def _check_store(case, st, ring_rows):
    exp = rs.case_expected(case)
    dup, offered, dropped = st.duplicates()
    eps, ep_offered, ep_dropped = st.episodes()
    assert dropped == 0 and ep_dropped == 0
    if not case.reflush:
        assert offered == 0                                                # cleaned mode: a trained agent records nothing more
    main_exp, dup_exp = rs.split_duplicates(exp)
    assert len(dup.r) == len(dup_exp.key) and len(ring_rows.r) == len(main_exp.key)
    stats = rs.check(exp, _cat(ring_rows, dup), eps)
    print("%s: %d rows (%d re-flush duplicates), %d episode records, %d returns differ from float32(oracle)"
          % (rs.case_id(case), stats["rows"], len(dup.r), stats["episodes"], stats["returns_differ"]))
    return stats


@pytest.mark.parametrize("case", rs.CASES, ids=[rs.case_id(c) for c in rs.CASES])
def test_push_matches_oracle_on_the_smallest_ring(case):
    st, ring_rows = _run_smallest_ring(case)
    _check_store(case, st, ring_rows)
    st.close()


NO_WRAP = rs.Case(33, 1, 0.97, **rs.SMALL)


def _run_no_wrap(case, **capacities):
    """a ring that never wraps: every step pushed, nothing compacted yet"""
    tl = rs.case_timeline(case)
    st = Store(case, ring_len=tl.T + 1, **capacities)
    for t in range(tl.T):
        st.push(t, t)
    return st


def test_push_matches_oracle_on_a_ring_that_never_wraps():
    """the same store through ONE flush_all-style compaction (mark_taken = 1) at the end; a second one finds nothing left"""
    case = NO_WRAP
    tl = rs.case_timeline(case)
    st = _run_no_wrap(case)
    total = tl.T * st.S
    out = st.new_out(total)
    offered, dropped = st.compact(0, tl.T, 1, out, 0, total)
    assert dropped == 0 and all(_intact(t, total) for t in out)
    _check_store(case, st, _rows(out, offered))
    assert st.compact(0, tl.T, 1, st.new_out(8), 0, 8) == (0, 0)
    st.close()


def test_device_side_step_counter_equals_explicit_steps():
    """step = -1 throughout: the handle's counter addresses the same blocks -- the rings bit-equal, the append buffers the same rows"""
    case = rs.Case(32, 1, 0.97, **rs.SMALL)
    a, rows_a = _run_smallest_ring(case)
    b, rows_b = _run_smallest_ring(case, device_counter=True)
    for name in ("x", "val", "ret", "act", "emit_t", "dup_count", "ep_count"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    _check_store(case, b, rows_b)

    def canon(rows):                                                       # arrival order of the atomics is not part of the result
        o = np.argsort(rs._pack(rows.src))
        return [np.asarray(v)[o] for v in rows]
    for rows_1, rows_2 in ((rows_a, rows_b), (a.duplicates()[0], b.duplicates()[0])):
        assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(canon(rows_1), canon(rows_2)))
    # (an episode's total_reward is a sum of double atomics whose order may differ from run to run: _check_store holds it to the oracle)
    ep = lambda s: sorted((int(e[0]), int(e[2])) for e in s.episodes()[0])
    assert ep(a) == ep(b)
    a.close(); b.close()


# ---- the three capacity paths --------------------------------------------------------------------------------------------------
CAP = rs.Case(2, 1, 0.97, **rs.SMALL)       # short buffers: thousands of re-flush duplicates, hundreds of episodes, in a short script


def _capacity(which, full):
    return 1 if which == "one" else full - 5


@pytest.mark.parametrize("which", ["one", "short"])
def test_duplicate_buffer_full(which):
    exp = rs.case_expected(CAP)
    main_exp, dup_exp = rs.split_duplicates(exp)
    Dn = len(dup_exp.key)
    cap = _capacity(which, Dn)
    assert 1 <= cap < Dn
    st = _run_no_wrap(CAP, dup_capacity=cap)
    dup, offered, dropped = st.duplicates()                                # (guard rows of the four tensors checked inside)
    assert (offered, dropped) == (Dn, Dn - cap) and len(dup.r) == cap
    rs.check(dup_exp, dup, subset=True)                                    # distinct members of the expected set; which: arrival order
    tl = rs.case_timeline(CAP)
    out = st.new_out(tl.T * st.S)
    offered, dropped = st.compact(0, tl.T, 0, out, 0, tl.T * st.S)
    assert dropped == 0
    eps, _, ep_dropped = st.episodes()
    assert ep_dropped == 0
    rs.check(main_exp, _rows(out, offered), eps)                           # the rings are none the worse
    st.close()


@pytest.mark.parametrize("which", ["one", "short"])
def test_episode_log_full(which):
    exp = rs.case_expected(CAP)
    En = len(exp.episodes)
    cap = _capacity(which, En)
    assert 1 <= cap < En
    st = _run_no_wrap(CAP, ep_capacity=cap)
    eps, offered, dropped = st.episodes()                                  # (guard rows checked inside)
    assert (offered, dropped) == (En, En - cap) and len(eps) == cap
    dup, _, dup_dropped = st.duplicates()
    assert dup_dropped == 0
    tl = rs.case_timeline(CAP)
    out = st.new_out(tl.T * st.S)
    offered, dropped = st.compact(0, tl.T, 0, out, 0, tl.T * st.S)
    assert dropped == 0
    rs.check(exp, _cat(_rows(out, offered), dup), eps, subset=True)        # distinct members of the expected records
    rs.check(exp, _cat(_rows(out, offered), dup))                          # and every row
    st.close()


@pytest.mark.parametrize("which", ["zero", "one", "short"])
def test_compaction_without_room(which):
    main_exp, _ = rs.split_duplicates(rs.case_expected(CAP))
    R = len(main_exp.key)
    cap = 0 if which == "zero" else _capacity(which, R)
    assert 0 <= cap < R
    tl = rs.case_timeline(CAP)
    st = _run_no_wrap(CAP)
    first = st.new_out(cap)
    assert st.compact(0, tl.T, 1, first, 0, cap) == (R, R - cap)
    assert all(_intact(t, cap) for t in first), "a write behind the compaction's capacity"
    rows_1 = _rows(first, cap)
    rs.check(main_exp, rows_1, subset=True)                                # distinct expected rows
    # mark_taken = 1 stamped exactly the rows that were stored: a second call with room returns the others, and only them
    second = st.new_out(R)
    assert st.compact(0, tl.T, 1, second, 0, R) == (R - cap, 0)
    assert all(_intact(t, R) for t in second)
    rs.check(main_exp, _cat(rows_1, _rows(second, R - cap)))               # the union: the expected set, no row twice
    assert st.compact(0, tl.T, 1, second, 0, R) == (0, 0)
    st.close()


# ---- the same paths through BatchedRollout ----------------------------------------------------------------------------------------
def _python_rollout(monkeypatch, fuse="0", steps=120, **kw):
    from rl_collision_avoidance_amd.ga3c.rollout import BatchedRollout
    from tests.gpu_support import _default_device_env as _make
    monkeypatch.setenv("CAVOID_FUSE_ENV_PUSH", fuse)
    W, N, seed = 96, 4, 3
    env = _make(W, N, seed, gen_min_agents=2, gen_nonlearning_fraction=0.3)
    kw.setdefault("reflush_done", True)
    roll = BatchedRollout(env, policy=None, time_max=5, discount=0.97, **kw)
    roll.reset()
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        acts = rng.integers(0, 11, size=(W, N)).astype(np.int32)
        acts[rng.random((W, N)) < 0.7] = 2
        vals = np.round(rng.normal(0, 0.5, size=(W, N)), 3).astype(np.float32)
        roll.step(torch.from_numpy(acts).cuda(), torch.from_numpy(vals).cuda())
    return env, roll


def _by_key(batch):
    x, r, a, src = (v.cpu().numpy() for v in (batch.x, batch.r, batch.a_index, batch.src))
    rows = {tuple(k): (x[i].tobytes(), r[i].tobytes(), int(a[i])) for i, k in enumerate(src)}
    assert len(rows) == len(r)
    return rows


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_batched_rollout_reports_what_a_full_buffer_dropped(fuse, monkeypatch):
    env, roll = _python_rollout(monkeypatch, fuse, ring_len=130, dup_capacity=1000000)
    n_dup, n_eps = int(roll.dup_count[0].item()), int(roll.ep_count[0].item())
    full = roll.drain(flush_all=True)
    everything, eps_all = _by_key(full), roll.drain_episodes().cpu().numpy()
    assert full.dropped == 0 and n_dup > 10 and n_eps > 10 and len(eps_all) == n_eps
    roll.close(); env.close()
    for cap, ep_cap in ((1, 1), (n_dup - 3, n_eps - 3)):
        env, roll = _python_rollout(monkeypatch, fuse, ring_len=130, dup_capacity=cap, episode_capacity=ep_cap)
        batch = roll.drain(flush_all=True)
        assert batch.dropped == n_dup - cap and len(batch) == len(full) - n_dup + cap       # the main rows plus `cap` duplicates
        got = _by_key(batch)
        assert all(everything[k] == v for k, v in got.items())
        assert int(roll.dup_count[0].item()) == 0
        assert roll.ep_count.tolist() == [n_eps, n_eps - ep_cap]
        eps = roll.drain_episodes().cpu().numpy()
        assert len(eps) == ep_cap == roll.episode_capacity
        assert roll.ep_count.tolist() == [0, 0]
        left = [tuple(e) for e in eps_all]
        for e in eps:                                 # distinct records of the full log (total_reward: a sum of atomics, to 1e-6)
            hit = [k for k, f in enumerate(left) if f[0] == e[0] and f[2] == e[2] and abs(f[1] - e[1]) <= 1e-6 * max(1.0, abs(f[1]))]
            assert hit, tuple(e)
            left.pop(hit[0])
        roll.close(); env.close()


def test_batched_rollout_counts_the_blocks_it_lost(monkeypatch):
    ring_len = 20
    env, late = _python_rollout(monkeypatch, "1", steps=ring_len + 5, ring_len=ring_len, reflush_done=False)
    batch = late.drain()
    assert late.lost_blocks == 5 and late.step_index == ring_len + 5
    assert len(batch) > 0 and int(batch.src[:, 2].min().item()) >= late.step_index - ring_len
    hi = late.step_index - late.margin
    late.close(); env.close()
    # a twin that drained in time, on the three-launch path
    env, twin = _python_rollout(monkeypatch, "0", steps=ring_len + 5, ring_len=64, reflush_done=False)
    in_time = twin.drain()
    assert twin.lost_blocks == 0 and twin.drained_until == hi
    want = {k: v for k, v in _by_key(in_time).items() if k[2] >= 5}
    assert _by_key(batch) == want and len(want) > 0
    twin.close(); env.close()
