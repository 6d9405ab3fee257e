"""CPU tests of the rest of the trainer step for the weight-sharing network (include/cavoid.h: cavoid_policy_param_layout_ws and the
scratch size of cavoid_policy_weight_grads_ws): the flat parameter layout against the module's parameters, and the Python restatement of
the row partition (the GPU tests' accumulation-chain length comes from it) against the header's constants and the library's own figure."""
import ctypes as C
import os
import re

import pytest

torch = pytest.importorskip("torch")

from tests.policy_regimes import build_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cavoid_policy_param_layout_ws", "cavoid_policy_weight_grads_scratch_ws", "cavoid_policy_weight_grads_ws", "cavoid_policy_apply_ws")


@pytest.mark.parametrize("M,A", [(1, 11), (7, 5), (19, 11), (64, 15)])
def test_param_layout_ws_is_the_modules_parameters(M, A):
    from rl_collision_avoidance_amd import _lib
    off, size, total = _lib.policy_param_layout_ws(M, A)
    names = _lib.POLICY_PARAM_NAMES_WS
    assert len(off) == len(size) == _lib.POLICY_PARAMS == len(names) == 12
    assert names == ("other_kernel", "other_bias", "layer1_kernel", "layer1_bias", "layer2_kernel", "layer2_bias", "fc1_kernel", "fc1_bias",
                     "p_kernel", "p_bias", "v_kernel", "v_bias")
    net = build_net("weight_sharing", M, A=A)
    params = dict(net.named_parameters())
    # the twelve variables are the module's parameters, each once; the sizes are matched by name (the module registers logits_v first)
    assert sorted(params) == sorted(names)
    assert size == [params[name].numel() for name in names]
    assert tuple(params["other_kernel"].shape) == (8, 64) and tuple(params["layer1_kernel"].shape) == (4 + 64 * M, 256)
    assert tuple(params["p_kernel"].shape) == (256, A)
    assert all(o % 64 == 0 for o in off) and off[0] == 0
    for i in range(11):
        assert off[i] + size[i] <= off[i + 1] < off[i] + size[i] + 64          # in order, no overlap, no more padding than the alignment needs
    assert total == off[11] + size[11]


def test_param_layout_ws_depends_on_max_other():
    from rl_collision_avoidance_amd import _lib
    assert _lib.policy_param_layout_ws(3, 11)[2] + 64 * 256 == _lib.policy_param_layout_ws(4, 11)[2]


def test_param_layout_ws_rejects_bad_arguments():
    from rl_collision_avoidance_amd import _lib
    lib = _lib.lib()
    off, size, total = (C.c_int64 * 12)(), (C.c_int64 * 12)(), C.c_int64()
    assert lib.cavoid_policy_param_layout_ws(3, 11, off, size, C.byref(total)) == 0
    assert lib.cavoid_policy_param_layout_ws(0, 11, off, size, C.byref(total)) == -1
    assert lib.cavoid_policy_param_layout_ws(65, 11, off, size, C.byref(total)) == -1
    assert lib.cavoid_policy_param_layout_ws(3, 0, off, size, C.byref(total)) == -1
    assert lib.cavoid_policy_param_layout_ws(3, 16, off, size, C.byref(total)) == -1
    assert lib.cavoid_policy_param_layout_ws(3, 11, None, size, C.byref(total)) == -1
    assert lib.cavoid_policy_param_layout_ws(3, 11, off, None, C.byref(total)) == -1
    assert lib.cavoid_policy_param_layout_ws(3, 11, off, size, None) == -1


def test_python_partition_ws_is_the_librarys():
    """policy_kernel.step_partition_ws restates cavoid_policy_step_ws.hpp's constants (held to the header's text), and the scratch size it
    gives is the header's formula.  The library's own figure needs a handle, hence a device: tests/test_gpu_policy_step_ws.py holds
    step_scratch_floats_ws to cavoid_policy_weight_grads_scratch_ws."""
    from rl_collision_avoidance_amd.ga3c import policy_kernel as pk
    text = open(os.path.join(ROOT, "rl_collision_avoidance_amd", "csrc", "cavoid_policy_step_ws.hpp")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int64_t (kStepWs\w+) = (\d+);", text)}
    assert (const["kStepWsL1Slice"], const["kStepWsFilterSlice"], const["kStepWsFilterSliceWide"], const["kStepWsFilterWideFrom"]) == \
        (pk.STEP_WS_L1_SLICE, pk.STEP_WS_FILTER_SLICE, pk.STEP_WS_FILTER_SLICE_WIDE, pk.STEP_WS_FILTER_WIDE_FROM)
    assert len(const) == 4                                 # (a slice constant this test does not know of would be one the mirror lacks)
    # (dense slices, layer1 slice length, layer1 slices, filter slice length, filter slices), worked out by hand from the header's table
    assert pk.step_partition_ws(3, 2112) == (3, 1024, 3, 1024, 7)
    assert pk.step_partition_ws(63, 16384) == (16, 1024, 16, 1024, 1008)
    assert pk.step_partition_ws(64, 65600) == (65, 1024, 65, 4096, 1025)
    assert pk.step_partition_ws(64, 65536)[3:] == (1024, 4096)           # exactly 4 194 304 flat rows: still the short slice
    assert pk.step_scratch_floats_ws(3, 2112) == 3 * 196 * 256 + 3 * 135168 + 7 * 512
    assert pk.step_scratch_floats_ws(63, 16384) == 16 * 4036 * 256 + 16 * 135168 + 1008 * 512
    assert pk.step_scratch_floats_ws(64, 65600) == 65 * 4100 * 256 + 65 * 135168 + 1025 * 512


def test_new_symbols_are_declared_bound_and_exported():
    """the header declares the four calls, the binding lists them, the library exports them (tests/test_host_cpu.py checks every declared symbol;
    this names the four)"""
    from rl_collision_avoidance_amd import _lib
    header = open(os.path.join(ROOT, "include", "cavoid.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    handle = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in bound, name
        assert getattr(handle, name) is not None, name
