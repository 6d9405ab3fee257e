"""The index algebra behind the mirrored pair distances (csrc/cavoid_kernels.hpp: mirror_computed, mirror_fetch), on the CPU.

Lane i's neighbour slot o is agent other(i, o) = (i + 1 + o) mod N.  The kernels compute the distance of the slots o < N / 2 and fetch
the others from the lane of that agent, slot N - 2 - o.  That is only right if (1) that slot of that lane points back at i, (2) the
slot fetched is one the mirror lane computes, every slot being either computed or fetched, and (3) both ends of a pair get the same
bits from their own subtraction: the squared distance is even in the differences."""
import numpy as np
import pytest

NS = list(range(2, 17))


def other(i, o, n):
    j = i + 1 + o
    return j - n if j >= n else j


def computed(n):
    """mirror_computed<N>() with CAVOID_MIRROR_DIST on: slots below it are computed (N = 2 has one slot, its own mirror)"""
    return n // 2 if n >= 3 else n - 1


@pytest.mark.parametrize("n", NS)
def test_the_mirror_of_a_slot_points_back(n):
    for i in range(n):
        seen = set()
        for o in range(n - 1):
            j, m = other(i, o, n), n - 2 - o
            assert j != i and 0 <= m <= n - 2
            assert other(j, m, n) == i                      # the mirror lane's slot is this pair
            assert other(i, n - 2 - m, n) == j              # ... and mirroring twice is the identity
            seen.add(j)
        assert seen == set(range(n)) - {i}


@pytest.mark.parametrize("n", NS)
def test_every_slot_is_computed_or_fetched_from_a_computed_one(n):
    own = computed(n)
    assert own == (n - 2) // 2 + 1 or n == 2                # slots o <= (N - 2) / 2, the self-mirrored middle slot of an even N among them
    fetched = list(range(own, n - 1))
    assert sorted(list(range(own)) + fetched) == list(range(n - 1))     # each slot exactly once
    for o in fetched:
        assert 0 <= n - 2 - o < own                         # what is fetched, the mirror lane has computed
    if n % 2 == 0:
        mid = (n - 2) // 2
        assert n - 2 - mid == mid and mid < own             # the middle slot mirrors itself and is computed
    # every unordered pair of a world is computed at least once, by the lower slot of its two ends
    pairs = set()
    for i in range(n):
        for o in range(own):
            pairs.add(frozenset((i, other(i, o, n))))
    assert len(pairs) == n * (n - 1) // 2


def test_quads_fetch_from_the_lane_before():
    """N = 4: slot 2 of lane i is slot 0 of lane (i + 3) mod 4 of the same quad: the DPP quad_perm [3, 0, 1, 2] (0x93)"""
    perm = [(0x93 >> (2 * k)) & 3 for k in range(4)]
    assert perm == [3, 0, 1, 2]
    assert computed(4) == 2
    for i in range(4):
        assert other(i, 2, 4) == perm[i] and 4 - 2 - 2 == 0


def test_the_squared_distance_is_even_in_its_differences_bit_for_bit():
    rng = np.random.default_rng(5)
    n = 200000
    parts = [rng.uniform(-20.0, 20.0, (4, n)),
             rng.uniform(-1.0, 1.0, (4, n)) * 2.0 ** rng.integers(-1074, -1000, (4, n)).astype(np.float64),     # denormal differences
             np.ldexp(rng.uniform(0.5, 1.0, (4, n)), rng.integers(-540, -500, (4, n))),                         # squares that underflow
             np.zeros((4, 8))]
    small = np.array([5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 0.0, -0.0, 1.0, -1.0])
    parts.append(np.stack([small, small[::-1], np.roll(small, 3), np.roll(small, 5)]))
    a, b, c, d = np.concatenate(parts, axis=1)
    with np.errstate(under="ignore"):
        lhs = (a - b) ** 2 + (c - d) ** 2
        rhs = (b - a) ** 2 + (d - c) ** 2
        lhs_mul = (a - b) * (a - b) + (c - d) * (c - d)
        rhs_mul = (b - a) * (b - a) + (d - c) * (d - c)
    assert np.array_equal(lhs.view(np.uint64), rhs.view(np.uint64))
    assert np.array_equal(lhs_mul.view(np.uint64), rhs_mul.view(np.uint64))
    assert np.array_equal(np.abs(a - b).view(np.uint64), np.abs(b - a).view(np.uint64))     # (a - b is -(b - a), or both are +0)
