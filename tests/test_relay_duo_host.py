"""The role table and the LDS layout of env_relay_kernel's two-tiles-per-workgroup form (csrc/cavoid_relay.hpp: relay_duo_slot,
relay_region_offset), on the CPU: the constexpr functions the kernel and the launcher use, called through the library's two host-only
entry points (cavoid_relay.hip).

A workgroup of 2 * (3 + NC + top-up) wavefronts owns two tiles; wavefront w runs on SIMD (first + w) mod 4, so the table is judged by
w mod 4: every role of both tiles exactly once, never a D and a P on one SIMD, the consumers dealt evenly.  Each tile's LDS region lies
behind the other's and the launch asks for exactly both."""
import ctypes as C

import pytest

D, P = 0, 1
CONSUMERS = (1, 2, 3, 4)                                    # CAVOID_RELAY_CONSUMERS' range (kRelayMaxConsumers)


@pytest.fixture(scope="module")
def lib():
    from rl_collision_avoidance_amd import build
    h = C.CDLL(build.build())
    h.cavoid_relay_duo_slot.restype, h.cavoid_relay_duo_slot.argtypes = C.c_int32, [C.c_int32] * 4
    h.cavoid_relay_lds_layout.restype, h.cavoid_relay_lds_layout.argtypes = C.c_int64, [C.c_int32] * 5
    return h


def _table(lib, nc, topup, mate):
    waves = 2 * (3 + nc + topup)
    slots = [lib.cavoid_relay_duo_slot(w, nc, topup, mate) for w in range(waves)]
    assert all(s >= 0 for s in slots), slots
    assert lib.cavoid_relay_duo_slot(waves, nc, topup, mate) == -1 and lib.cavoid_relay_duo_slot(-1, nc, topup, mate) == -1
    return [(s >> 4, s & 15) for s in slots]                # (tile, role)


@pytest.mark.parametrize("mate", [0, 1, -1], ids=["own", "other", "built"])
@pytest.mark.parametrize("topup", [0, 1])
@pytest.mark.parametrize("nc", CONSUMERS)
def test_role_table(lib, nc, topup, mate):
    table = _table(lib, nc, topup, mate)
    assert len(table) <= 16                                 # one workgroup: at most 1024 threads
    roles = 3 + nc + topup                                  # D, P, the consumers, L (, T): numbered as for one tile per workgroup
    assert sorted(table) == [(t, r) for t in (0, 1) for r in range(roles)]     # every role of both tiles exactly once, nothing else
    consumers = [0, 0, 0, 0]
    for simd in range(4):
        here = [r for w, (t, r) in enumerate(table) if w % 4 == simd]
        assert sum(1 for r in here if r in (D, P)) <= 1, (simd, here)
        consumers[simd] = sum(1 for r in here if 2 <= r < 2 + nc)
    assert max(consumers) - min(consumers) <= 1, consumers
    # the chain wavefronts are the first four, one per SIMD, whatever the rest of the launch looks like (relay_coop_last reads the role
    # of D and P off the wavefront index), and the loaders sit right behind the consumers
    assert table[:4] == [(0, D), (1, D), (0, P), (1, P)]
    assert sorted(table[4 + 2 * nc:6 + 2 * nc]) == [(0, 2 + nc), (1, 2 + nc)]
    # a launch without the top-up is the launch with it minus its LAST two wavefronts: nobody else changes SIMD
    if topup:
        assert table[:-2] == _table(lib, nc, 0, mate) and sorted(table[-2:]) == [(0, 3 + nc), (1, 3 + nc)]


def test_four_consumers_fill_every_simd_alike(lib):
    table = _table(lib, 4, 1, -1)
    for simd in range(4):
        here = sorted(r for w, (t, r) in enumerate(table) if w % 4 == simd)
        chain, rest = here[0], here[1:]
        assert chain in (D, P) and sum(1 for r in rest if 2 <= r < 6) == 2 and sum(1 for r in rest if r >= 6) == 1, (simd, here)


def test_the_two_candidate_tables_differ_only_in_whose_consumers_sit_where(lib):
    for nc in CONSUMERS:
        own, other = _table(lib, nc, 1, 0), _table(lib, nc, 1, 1)
        for w, ((t0, r0), (t1, r1)) in enumerate(zip(own, other)):
            assert r0 == r1 and (t0 != t1) == (2 <= r0 < 2 + nc), (nc, w)
        # "own": the consumers on D's and P's SIMD belong to that wavefront's tile
        for w, (t, r) in enumerate(own):
            if 2 <= r < 2 + nc:
                assert t == own[w % 4][0], (nc, w)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_lds_regions(lib, n):
    for nc in CONSUMERS:
        for tile_floats in (4, 28, 64 * (6 + 7 * (n - 1) + 2), 4 * 463):
            region = lib.cavoid_relay_lds_layout(n, 1, nc, tile_floats, 3)
            assert region > 0 and region % 16 == 0          # (the rings and the tiles are read 16 bytes at a time)
            assert lib.cavoid_relay_lds_layout(n, 1, nc, tile_floats, 2) == region
            assert lib.cavoid_relay_lds_layout(n, 2, nc, tile_floats, 2) == 2 * region
            off = [lib.cavoid_relay_lds_layout(n, 2, nc, tile_floats, t) for t in (0, 1)]
            assert off == [0, region]                       # [0, region) and [region, 2 region): no overlap, nothing unused
            assert off[1] + region == lib.cavoid_relay_lds_layout(n, 2, nc, tile_floats, 2)
            assert region - nc * tile_floats * 4 == lib.cavoid_relay_lds_layout(n, 1, 0, tile_floats, 3)     # the fixed part + nc tiles
    assert lib.cavoid_relay_lds_layout(7, 2, 3, 64, 2) == -1                      # not an agent count of the relay
