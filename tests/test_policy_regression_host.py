"""CPU side of tests/test_gpu_policy_regression.py (the supervised start on the fused trainer kernels): the two new C calls are declared
in plain C, exported and bound; the built library's regression kernels use no scratch; and, from the same table the GPU file runs
(tests/regression_regimes.py), with float64 autograd alone: every case meets its conditions, the head written out the way the kernels
compute it is the gradient of ``regression_loss``, and each wrong head the regimes exist to catch moves some gradient by at least 100x
the bound the GPU criterion allows."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

torch = pytest.importorskip("torch")

from tests import regression_regimes as G
from tests.host_support import LLVM, ROOT, _kernel_notes

NEW_SYMBOLS = ("cavoid_policy_train_regression", "cavoid_policy_train_regression_ws")
HEADER = os.path.join(ROOT, "include", "cavoid.h")


def test_new_calls_are_declared_in_plain_c_exported_and_bound():
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert "NetworkVPCore.py:90-100,123" in text
    assert re.search(r"#define\s+CAVOID_ABI_VERSION\s+3\b", text)
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:                                        # the header still compiles as C, and the calls take the A3C pair's buffer structs
        work = tempfile.mkdtemp(prefix="cavoid_hdr_")
        try:
            src = os.path.join(work, "t.c")
            with open(src, "w") as f:
                f.write('#include "cavoid.h"\n'
                        "int (*lstm)(cavoid_policy *, const float *, int64_t, int64_t, const float *, const int32_t *,\n"
                        "            const cavoid_policy_train_buffers *, void *) = cavoid_policy_train_regression;\n"
                        "int (*ws)(cavoid_policy *, const float *, int64_t, int64_t, const float *, const int32_t *,\n"
                        "          const cavoid_policy_train_ws_buffers *, void *) = cavoid_policy_train_regression_ws;\n")
            subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.dirname(HEADER), "-c", src, "-o",
                            os.path.join(work, "t.o")], check=True)
        finally:
            shutil.rmtree(work, ignore_errors=True)
    from rl_collision_avoidance_amd import _lib
    lib = _lib.lib()
    bound = {name: (restype, argtypes) for name, restype, argtypes in _lib.SYMBOLS}
    for name, a3c, buffers in (("cavoid_policy_train_regression", "cavoid_policy_train", _lib.CavoidPolicyTrainBuffers),
                               ("cavoid_policy_train_regression_ws", "cavoid_policy_train_ws", _lib.CavoidPolicyTrainWsBuffers)):
        assert hasattr(lib, name) and name in bound, name
        # the A3C call's arguments without beta and log_epsilon
        assert bound[name][0] is C.c_int and bound[name][1] == [t for t in bound[a3c][1] if t is not C.c_float]
        assert bound[name][1][6] == C.POINTER(buffers)


def test_without_a_handle_they_return_what_the_a3c_calls_return():
    """the first check of all four calls: no handle (what a box without a device is left with, cavoid_policy_create having failed)
    and a wrong struct_size are error codes, not crashes"""
    from rl_collision_avoidance_amd import _lib
    lib = _lib.lib()
    x = (C.c_float * 64)()
    a = (C.c_int32 * 4)()
    for new, old, struct in ((lib.cavoid_policy_train_regression, lib.cavoid_policy_train, _lib.CavoidPolicyTrainBuffers),
                             (lib.cavoid_policy_train_regression_ws, lib.cavoid_policy_train_ws, _lib.CavoidPolicyTrainWsBuffers)):
        b = struct()
        for size in (C.sizeof(struct), 8):
            b.struct_size, b.capacity_rows = size, 64
            want = old(None, x, 4, 16, x, a, 1e-4, 1e-6, C.byref(b), None)
            assert want == -1                        # CAVOID_EINVAL
            assert new(None, x, 4, 16, x, a, C.byref(b), None) == want


@pytest.mark.skipif(not (os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))),
                    reason="llvm-objdump / llvm-readelf of the ROCm toolchain not present")
def test_regression_kernels_use_no_scratch():
    text = _kernel_notes()
    found = re.findall(r"\.name:\s+(\S*policy_regression_\S*kernel\S*)\s*\n\s*\.private_segment_fixed_size:\s+(\d+)", text)
    assert len(found) == 2, found            # the LSTM network's and the weight-sharing network's trainer forward
    assert all(int(size) == 0 for _, size in found), found


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_every_gpu_case_meets_its_conditions(case):
    net, x, y, a, info = G.build_case(case)
    assert x.shape == (case.B, net.input_size) and y.shape == a.shape == (case.B,) and net.min_policy == case.min_policy
    print("%s: the row filter excludes %.2f %% of the candidates, %.1f %% of the rows select a float32 probability of exactly 0"
          % (G.case_id(case), 100.0 * info["excluded"], 100.0 * info["zero_selected"]))
    G.assert_conditions(case, info)


HOST_CASES = [c for c in G.CASES if c.B == 1000]
MUTATION_OF = {"fresh": ("no_value_term",), "min_policy": ("min_policy_softmax", "no_value_term"),
               "gain40": ("a3c_log_clamp", "no_value_term"), "gain150": ("a3c_log_clamp", "no_value_term")}


@pytest.mark.parametrize("case", HOST_CASES, ids=G.case_id)
def test_the_written_out_head_is_the_gradient_of_regression_loss(case):
    net, x, y, a, _ = G.build_case(case)
    cost_p, cost_v, want, torch32 = G.reference_gradients(net, x, y, a)
    assert all(torch.isfinite(g).all() for g in torch32.values())          # (PyTorch's float32 stays finite in every regime)
    got = G.head_gradients(net, x, y, a)
    for k, ref in want.items():
        assert (got[k] - ref).abs().max().item() <= 1e-9 * (ref.abs().max().item() + 1e-6), k
    # ... and the two sums in the log-sum-exp form the kernels take: log s + m - z_a, 0.5 (y - v)^2
    with torch.no_grad():
        z, _, v = net.double().forward(x.double())
    m = z.max(dim=1).values
    lse = torch.log(torch.exp(z - m[:, None]).sum(dim=1)) + m - z.gather(1, a.unsqueeze(1)).squeeze(1)
    assert abs(lse.sum().item() - cost_p) <= 1e-9 * max(1.0, abs(cost_p))
    assert abs(0.5 * ((y.double() - v) ** 2).sum().item() - cost_v) <= 1e-9 * max(1.0, abs(cost_v))


@pytest.mark.parametrize("case", HOST_CASES, ids=G.case_id)
def test_a_wrong_head_would_move_the_gradients(case):
    """cross-entropy on the MIN_POLICY-floored softmax (min_policy regime), the A3C head's LOG_EPSILON clamp (gain 40 and 150), no
    value term (every regime): each moves some gradient by at least 100x what assert_gradients_match allows on this batch"""
    net, x, y, a, _ = G.build_case(case)
    _, _, want, torch32 = G.reference_gradients(net, x, y, a)
    for mutation in MUTATION_OF[case.regime]:
        ratio = G.worst_ratio(G.head_gradients(net, x, y, a, mutation), want, torch32)
        print("%s: %s moves a gradient by %.0f x the criterion's bound" % (G.case_id(case), mutation, ratio))
        assert ratio >= 100.0, (case, mutation, ratio)
