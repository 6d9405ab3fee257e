"""CPU tests of the rest of the trainer step (include/cavoid.h: cavoid_policy_param_layout, cavoid_policy_optimizer): the flat parameter
layout against the module's parameters, the new structs as plain C99 with the binding's mirrors at the compiler's sizes, and the float64
restatements of the update rules (tests/policy_step_rules.py, the yardstick of tests/test_gpu_policy_step.py) against something that is
not themselves."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

torch = pytest.importorskip("torch")

from tests import policy_step_rules as rules
from tests.policy_regimes import build_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("M,A", [(3, 11), (19, 11), (63, 5)])
def test_param_layout_is_the_modules_parameters(M, A):
    from rl_collision_avoidance_amd import _lib
    off, size, total = _lib.policy_param_layout(M, A)
    assert len(off) == len(size) == _lib.POLICY_PARAMS == len(_lib.POLICY_PARAM_NAMES) == 12
    net = build_net("rnn", M, A=A)
    params = dict(net.named_parameters())
    # the twelve variables are the module's parameters, each once; the ORDER is cavoid_policy_weights' (logits_p before logits_v; the
    # module registers logits_v first), so the sizes are matched by name
    assert sorted(params) == sorted(_lib.POLICY_PARAM_NAMES)
    assert size == [params[name].numel() for name in _lib.POLICY_PARAM_NAMES]
    weights_fields = [n for n, _ in _lib.CavoidPolicyWeights._fields_ if n.endswith(("_kernel", "_bias")) and n != "forget_bias"]
    assert weights_fields == list(_lib.POLICY_PARAM_NAMES)
    assert all(o % 64 == 0 for o in off) and off[0] == 0
    for i in range(11):
        assert off[i] + size[i] <= off[i + 1] < off[i] + size[i] + 64          # in order, no overlap, no more padding than the alignment needs
    assert total == off[11] + size[11]


def test_param_layout_rejects_bad_arguments():
    from rl_collision_avoidance_amd import _lib
    lib = _lib.lib()
    off, size, total = (C.c_int64 * 12)(), (C.c_int64 * 12)(), C.c_int64()
    assert lib.cavoid_policy_param_layout(0, 11, off, size, C.byref(total)) == -1
    assert lib.cavoid_policy_param_layout(65, 11, off, size, C.byref(total)) == -1
    assert lib.cavoid_policy_param_layout(3, 16, off, size, C.byref(total)) == -1
    assert lib.cavoid_policy_param_layout(3, 11, None, size, C.byref(total)) == -1
    assert lib.cavoid_policy_param_layout(3, 11, off, size, None) == -1


def test_new_structs_are_plain_c_and_mirrored(tmp_path):
    """the method of tests/test_host_cpu.py::test_header_is_plain_c on the structs this header gained"""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "hdr.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cavoid.h"\nint main(void) { cavoid_policy_optimizer o; cavoid_policy_weights w;\n'
                   '  (void)o; (void)w; printf("%d %d %d %d %d %d\\n", (int)sizeof(o), (int)sizeof(w), (int)offsetof(cavoid_policy_optimizer, lr),\n'
                   '  (int)offsetof(cavoid_policy_optimizer, clip_average_norm), (int)offsetof(cavoid_policy_optimizer, step), CAVOID_POLICY_PARAMS);\n'
                   '  return 0; }\n')
    exe = tmp_path / "hdr"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    from rl_collision_avoidance_amd import _lib
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    o = _lib.CavoidPolicyOptimizer
    assert got == [C.sizeof(o), C.sizeof(_lib.CavoidPolicyWeights), o.lr.offset, o.clip_average_norm.offset, o.step.offset, _lib.POLICY_PARAMS]


def test_python_partition_is_the_librarys():
    """policy_kernel.step_partition (the tests' accumulation-chain length comes from it) restates cavoid_policy_step.hpp's constants: held to
    the header's text"""
    import re
    from rl_collision_avoidance_amd.ga3c import policy_kernel as pk
    text = open(os.path.join(ROOT, "rl_collision_avoidance_amd", "csrc", "cavoid_policy_step.hpp")).read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int64_t (kStep\w+) = (\d+);", text)}
    assert (const["kStepDenseSlice"], const["kStepLstmSlice"], const["kStepLstmSliceWide"], const["kStepLstmWideFrom"]) == \
        (pk.STEP_DENSE_SLICE, pk.STEP_LSTM_SLICE, pk.STEP_LSTM_SLICE_WIDE, pk.STEP_LSTM_WIDE_FROM)
    assert pk.step_partition(3, 2112) == (3, 1024, 7) and pk.step_partition(63, 16384) == (16, 1024, 1008) and pk.step_partition(64, 65600) == (65, 4096, 1025)


def _tensors(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g, dtype=torch.float64) * scale for shape in ((7, 5), (33,), (1,))]


def test_adam_restatement_is_torch_adam():
    """four steps, another lr each step, on float64 CPU tensors: 1e-12 relative"""
    lrs = [1e-3, 3e-4, 2e-3, 5e-5]
    w0 = _tensors(1)
    grads = [_tensors(10 + t, scale=0.3) for t in range(4)]
    params = [torch.nn.Parameter(t.clone()) for t in w0]
    opt = torch.optim.Adam(params, lr=lrs[0], eps=1e-8)
    for t, lr in enumerate(lrs):
        opt.param_groups[0]["lr"] = lr
        for p, g in zip(params, grads[t]):
            p.grad = g.clone()
        opt.step()
    w, m, v = rules.run_steps("adam", w0, grads, lrs)
    for i, p in enumerate(params):
        st = opt.state[p]
        for got, want in ((w[i], p.detach()), (m[i], st["exp_avg"]), (v[i], st["exp_avg_sq"])):
            assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_rmsprop_restatement_is_torch_rmsprop_where_the_two_rules_coincide(momentum):
    """eps = 0 and a constant lr: TensorFlow's eps-inside-the-root and lr-inside-the-momentum rule is PyTorch's.  square_avg preset to ones."""
    lr, steps = 1e-3, 4
    w0 = _tensors(2)
    grads = [_tensors(20 + t, scale=0.3) for t in range(steps)]
    params = [torch.nn.Parameter(t.clone()) for t in w0]
    opt = torch.optim.RMSprop(params, lr=lr, alpha=0.99, eps=0.0, momentum=momentum, centered=False)
    for t in range(steps):
        for p, g in zip(params, grads[t]):
            p.grad = g.clone()
        if t == 0:                                   # (the state exists from the first step on: preset it by stepping on ones)
            for p in params:
                opt.state[p] = {"step": torch.tensor(0.0), "square_avg": torch.ones_like(p)}
                if momentum > 0:
                    opt.state[p]["momentum_buffer"] = torch.zeros_like(p)
        opt.step()
    w, ms, mom = rules.run_steps("rmsprop", w0, grads, [lr] * steps, decay=0.99, momentum=momentum, eps=0.0)
    for i, p in enumerate(params):
        assert (w[i] - p.detach()).abs().max().item() <= 1e-12 * p.detach().abs().max().item()
        assert (ms[i] - opt.state[p]["square_avg"]).abs().max().item() <= 1e-12 * opt.state[p]["square_avg"].abs().max().item()
        if momentum > 0:                             # TensorFlow's accumulator carries the lr: lr * PyTorch's buffer
            assert (mom[i] - lr * opt.state[p]["momentum_buffer"]).abs().max().item() <= 1e-12 * mom[i].abs().max().item()


def test_clip_restatement_is_the_closed_form():
    g = torch.tensor([3.0, -4.0, 0.0, 12.0], dtype=torch.float64)         # ||g|| = 13, n = 4: average norm 3.25
    assert rules.average_norm(g) == 3.25
    above = rules.clip_by_average_norm(g, 2.0)                            # above c: scaled by c / 3.25, the average norm becomes c
    assert torch.allclose(above, g * (2.0 / 3.25), rtol=1e-15, atol=0.0) and abs(rules.average_norm(above) - 2.0) <= 1e-15
    below = rules.clip_by_average_norm(g, 5.0)                            # below c: untouched, bit for bit
    assert torch.equal(below, g)
