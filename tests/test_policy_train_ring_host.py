"""CPU tests of the crowd trainer's host side: the ring kernels in the built library (zero scratch), the Python limits and the scratch
figure, the training CLI's flag, and the exactness of the rollout compaction's multiply-shift division on wide rows."""
import os
import re

import pytest

from tests.host_support import LLVM, ROOT, _kernel_notes

CSRC = os.path.join(ROOT, "rl_collision_avoidance_amd", "csrc")


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))),
                    reason="llvm-objdump / llvm-readelf of the ROCm toolchain not present")
def test_ring_kernels_exist_and_use_no_scratch():
    text = _kernel_notes()
    found = dict(re.findall(r"\.name:\s+(\S*policy_train_ring_\w+_kernel\S*)\s*\n\s*\.private_segment_fixed_size:\s+(\d+)", text))
    assert len(found) == 2, found
    assert any("policy_train_ring_forward_kernel" in k for k in found) and any("policy_train_ring_regression_kernel" in k for k in found)
    assert all(int(size) == 0 for size in found.values()), found
    # the names stay clear of the substrings other tests count kernels by
    assert not any("crowd_kernel" in k or "policy_crowd_forward_kernel" in k for k in found)


def test_neighbour_limits_mirror_the_kernels():
    from rl_collision_avoidance_amd.ga3c.policy_kernel import MAX_OTHERS, MAX_OTHERS_INFERENCE, MAX_OTHERS_TRAIN
    assert MAX_OTHERS_TRAIN == 64 and MAX_OTHERS == 19 and MAX_OTHERS_TRAIN <= MAX_OTHERS_INFERENCE
    src = open(os.path.join(CSRC, "cavoid_policy_train_ring.hpp")).read()
    m = re.search(r"constexpr\s+int\s+kPolMaxOthersTrain\s*=\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) == MAX_OTHERS_TRAIN
    assert re.search(r"constexpr\s+int\s+kPolTrainRing\s*=\s*kPolMaxOthers\s*;", src)


def test_scratch_bytes():
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    assert FusedA3CTrainer.scratch_bytes(63, 16384) == 16384 * (6496 + 3360 * 63)
    assert FusedA3CTrainer.scratch_bytes(19, 64, arch="rnn") == 64 * (6496 + 3360 * 19)
    # the figure is _scratch's own shapes: per buffer row z1..z3 g1..g3 gh l1_in, per row and neighbour h_in save gl (float32)
    M = 31
    per_row = 4 * (6 * 256 + 16 + 72) + 4 * M * (72 + 16 * 256 * 8 // 64 + 256)
    assert FusedA3CTrainer.scratch_bytes(M, 1) == per_row
    assert FusedA3CTrainer.scratch_bytes(7, 1, arch="weight_sharing") == 4 * (6 * 256 + 16 + 4 + 64 * 7) + 4 * 7 * (8 + 64)
    assert [FusedA3CTrainer.buffer_rows(n) for n in (1, 64, 65, 2047, 2048, 2049)] == [64, 64, 128, 2048, 2048, 4096]


def test_train_cli_knows_the_flag(monkeypatch):
    """the parser accepts --fused-crowd-trainer (off by default); parsing stops before anything touches a device"""
    import argparse
    from rl_collision_avoidance_amd.ga3c import train
    seen = {}

    class Stop(Exception):
        pass

    def parse(self, argv=None):
        seen["args"] = argparse.ArgumentParser.parse_known_args(self, argv)[0]
        raise Stop()
    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse)
    for argv, want in ((["--fused-crowd-trainer"], True), ([], False)):
        with pytest.raises(Stop):
            train.main(argv)
        assert seen["args"].fused_crowd_trainer is want
    monkeypatch.undo()
    with pytest.raises(SystemExit):                          # (an unknown flag is still an error)
        train.main(["--fused-crowd-trainers-typo"])


def _compaction_constants():
    """(rows a wavefront copies at most, the over-run of its last trip, the refusal's limit) read from the sources: the copy loop's
    shape in cavoid_rollout.hpp and the limit cavoid_rollout_compact proves in its comment"""
    hpp = open(os.path.join(CSRC, "cavoid_rollout.hpp")).read()
    capi = open(os.path.join(CSRC, "cavoid_rollout_capi.hip")).read()
    span = int(re.search(r"constexpr\s+int\s+kCompactSpan\s*=\s*(\d+)\s*;", hpp).group(1))
    assert "const uint32_t inv_d = (uint32_t)((1ull << 32) / (uint32_t)D) + 1u;" in hpp
    assert "(int)(((uint64_t)(uint32_t)e * inv_d) >> 32)" in hpp
    assert "inv_d = floor(2^32 / D) + 1" in capi and "exact while e D < 2^32" in capi
    m = re.search(r"if \(\(64 \* kCompactSpan \* D \+ (\d+)\) \* D >= \(1ull << 32\)\) return CAVOID_EUNSUPPORTED;", capi)
    assert m
    return 64 * span, int(m.group(1))


@pytest.mark.parametrize("D", [255, 257, 446, 453])
def test_compaction_quotient_is_exact(D):
    """(e * inv_d) >> 32 == e // D for every element index the copy loop forms: e < 256 D and the masked lanes of the last trip"""
    import numpy as np
    rows, overrun = _compaction_constants()
    assert rows == 256 and overrun >= 64 * 8 - 1
    inv_d = (1 << 32) // D + 1
    assert inv_d < 1 << 32
    e = np.arange(rows * D + overrun, dtype=np.uint64)
    assert e[-1] * D < 1 << 32                               # the proof's condition ...
    assert np.array_equal((e * np.uint64(inv_d)) >> np.uint64(32), e // np.uint64(D))     # ... and the claim, exhaustively
    assert (rows * D + overrun) * D < 1 << 32                # the call accepts this width


def test_compaction_limit_is_where_the_proof_ends():
    rows, overrun = _compaction_constants()
    accepted = [D for D in range(1, 5000) if (rows * D + overrun) * D < 1 << 32]
    assert accepted == list(range(1, accepted[-1] + 1)) and accepted[-1] >= 453
    D = accepted[-1]
    inv_d = (1 << 32) // D + 1
    for e in (rows * D + overrun - 1, rows * D - 1, D * (rows - 1), D * rows):
        assert (e * inv_d) >> 32 == e // D
