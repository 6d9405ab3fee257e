"""The rest of the trainer step inside the library for the WEIGHT-SHARING network (include/cavoid.h: cavoid_policy_weight_grads_ws,
cavoid_policy_apply_ws) and its opt-in use from FusedA3CTrainer(ws_device_step=True) and ga3c.train --ws-device-step.

Yardsticks, none of them the code under test, as in tests/test_gpu_policy_step.py: the gradients are held to float64 autograd by the
criterion of test_fused_trainer_gradients_match_autograd (tests/policy_regimes.py: the one copy) and, on the raw binding, to float64
X^T G of the downloaded buffers; the optimiser to the float64 restatements of tests/policy_step_rules.py (which
tests/test_policy_step_host.py holds to torch.optim on float64 CPU tensors); the re-pack to a fresh load of the updated module."""
import copy
import ctypes as C
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

from tests import policy_step_rules as rules
from tests.policy_regimes import assert_gradients_match, build_net, inputs, reference_gradients

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -4
U = 2.0 ** -24                          # float32 unit roundoff
WS = "weight_sharing"


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _clone(s):
    """a copy of a ctypes struct (structs with pointer fields do not pickle, so copy.copy refuses them)"""
    c = type(s)()
    C.memmove(C.byref(c), C.byref(s), C.sizeof(s))
    return c


def _batch(net, B, seed):
    x = inputs(net, B, seed=seed)
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, generator=g).to(x.device)
    a = torch.randint(0, net.num_actions, (B,), generator=g).to(x.device)
    return x, y, a


def _trainer(net, **kw):
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    return FusedA3CTrainer(net, ws_device_step=True, ws_crowd=net.max_others > 19, **kw)


def _padding(off, size, total):
    pad = torch.ones(total, dtype=torch.bool, device="cuda")
    for o, n in zip(off, size):
        pad[o:o + n] = False
    return pad


# ---- gradients ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,B,min_policy", [(1, 130, 0.0), (3, 64, 0.0), (3, 1000, 1e-3), (7, 2112, 0.0), (19, 2112, 0.0), (20, 100, 0.0)])
def test_ws_device_step_gradients_match_autograd(M, B, min_policy):
    """cavoid_policy_train_ws + cavoid_policy_weight_grads_ws against float64 autograd, by test_fused_trainer_gradients_match_autograd's
    criterion and test_device_step_gradients_match_autograd's loss bound.  M = 1: layer1 is the host edge plus one block; B = 2112: buffers
    of 4096 rows, several slices, most of the last one zero rows; M = 20: a ring handle."""
    net = build_net(WS, M, seed=20 + M, min_policy=min_policy).cuda()
    x, y, a = _batch(net, B, seed=B + 1)
    total, _, _, want, torch32 = reference_gradients(net, x, y, a)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    tr = _trainer(net, learning_rate=0.0)
    assert tr.device_step and tr.ws_crowd == (M > 19)
    loss = float(tr.train(x, y, a))
    assert abs(loss - total) <= 2e-4 * max(1.0, abs(total))
    report = []
    assert_gradients_match(net, want, torch32, B, report=report)
    print([(k, "%.3g" % e, "%.3g" % e32) for k, e, e32, _ in report])
    for k, v in net.named_parameters():                    # lr = 0: the optimiser step leaves the masters alone, bit for bit
        assert torch.equal(v.detach(), before[k]), k


def _products(d, M, R, A, absolute=False):
    """{name: float64 X^T G of the downloaded buffers in the checkpoint's layout} (nothing is permuted), the biases from db"""
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    xtg = lambda X, G: f(X).t() @ f(G)
    head = xtg(d["z3"], d["gh"])
    db = torch.zeros_like(d["db"]) if absolute else d["db"]
    return {"other_kernel": xtg(d["f_in"].view(M * R, 8), d["gf"].view(M * R, 64)), "other_bias": db[:64],
            "layer1_kernel": xtg(d["l1_in"], d["g1"]), "layer1_bias": db[256:512], "layer2_kernel": xtg(d["z1"], d["g2"]), "layer2_bias": db[512:768],
            "fc1_kernel": xtg(d["z2"], d["g3"]), "fc1_bias": db[768:1024], "p_kernel": head[:, :A], "p_bias": db[1024:1024 + A],
            "v_kernel": head[:, A:A + 1], "v_bias": db[1024 + A:1025 + A]}


@pytest.mark.parametrize("M,A,R,B", [(3, 11, 2112, 2100), (20, 11, 128, 50)])
def test_raw_binding_products_at_a_capacity_buffer_rows_never_makes(M, A, R, B):
    """capacity_rows = 2112 (a multiple of 64, not of 2048: three slices, the last of 64 rows) and 128 on a ring handle, through the raw
    calls, scratch and grads_flat pre-filled with NaN: the five products against float64 X^T G of the downloaded buffers, entrywise within
    n u (|X|^T |G|), n the longest accumulation chain (slice length + number of partials), u = 2^-24: the bound of a float32 fma chain.  A
    dropped slice, a shifted layer1 block or a swapped host edge misses it by orders of magnitude."""
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer, step_partition_ws, step_scratch_floats_ws
    net = build_net(WS, M, seed=23, A=A).cuda()
    tr = _trainer(net, learning_rate=0.0)
    pol, lib = tr.policy, _lib.lib()
    x, y, a = _batch(net, B, seed=5)
    t, cbuf = tr._scratch(R)
    assert cbuf.capacity_rows == R and FusedA3CTrainer.buffer_rows(B) != R
    _lib.check(lib.cavoid_policy_train_ws(pol._h, _ptr(x), B, x.stride(0), _ptr(y), _ptr(a.to(torch.int32)), float(net.beta), float(net.log_epsilon),
                                          C.byref(cbuf), pol._stream()), "cavoid_policy_train_ws")
    floats = C.c_int64()
    _lib.check(lib.cavoid_policy_weight_grads_scratch_ws(pol._h, R, C.byref(floats)), "scratch")
    dense, l1_len, l1, f_len, f = step_partition_ws(M, R)
    assert floats.value == step_scratch_floats_ws(M, R) == l1 * (4 + 64 * M) * 256 + dense * (2 * 65536 + 256 * 16) + f * 512
    scratch = torch.full((floats.value,), float("nan"), device="cuda")
    off, size, total = _lib.policy_param_layout_ws(M, A)
    flat = torch.full((total,), float("nan"), device="cuda")
    _lib.check(lib.cavoid_policy_weight_grads_ws(pol._h, C.byref(cbuf), _ptr(scratch), scratch.numel(), _ptr(flat), pol._stream()), "weight_grads_ws")
    d = {k: v.double() for k, v in t.items()}
    want, mag = _products(d, M, R, A), _products(d, M, R, A, absolute=True)
    n = max(min(R, 1024) + dense, min(R, l1_len) + l1, min(M * R, f_len) + f)
    print("accumulation chain n = %d (dense %d slices, layer1 %d of %d, filter %d of %d)" % (n, dense, l1, l1_len, f, f_len))
    for name, o, sz in zip(_lib.POLICY_PARAM_NAMES_WS, off, size):
        got = flat[o:o + sz].double().view_as(want[name])
        assert torch.isfinite(got).all(), name
        if name.endswith("_bias"):                         # db itself, moved
            assert torch.equal(got, want[name]), name
            continue
        excess = ((got - want[name]).abs() - n * U * mag[name]).max().item()
        print(name, "max |err| %.3g, max bound %.3g" % ((got - want[name]).abs().max().item(), (n * U * mag[name]).max().item()))
        assert excess <= 0.0, (name, excess)
        assert want[name].abs().max().item() > 0.0, name
    assert torch.isfinite(flat).all() and (flat[_padding(off, size, total)] == 0.0).all()


@pytest.mark.parametrize("M,rows", [(3, 2112), (63, 16384), (64, 65600)])
def test_python_partition_ws_is_the_librarys_scratch_figure(M, rows):
    """policy_kernel.step_scratch_floats_ws against cavoid_policy_weight_grads_scratch_ws on a handle (tests/test_policy_step_ws_host.py holds
    the partition to the header's constants; the library's figure needs a handle).  No buffer is allocated."""
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.ga3c.policy_kernel import step_scratch_floats_ws
    lib, h, floats = _lib.lib(), C.c_void_p(), C.c_int64()
    create = lib.cavoid_policy_create_ws_crowd if M > 19 else lib.cavoid_policy_create_ws
    _lib.check(create(M, 11, 0, C.byref(h)), "create")
    try:
        _lib.check(lib.cavoid_policy_weight_grads_scratch_ws(h, rows, C.byref(floats)), "scratch")
        assert floats.value == step_scratch_floats_ws(M, rows)
    finally:
        lib.cavoid_policy_destroy(h)


def test_weight_grads_ws_twice_gives_the_same_bits_and_zero_padding():
    net = build_net(WS, 3, seed=24).cuda()
    tr = _trainer(net, learning_rate=0.0)
    x, y, a = _batch(net, 4160, seed=6)
    t = tr._pass(x, y, a.to(torch.int32), 4160)
    first = tr._flat_grads.clone()
    tr._flat_grads.fill_(float("nan"))                     # (the second call writes every float, the padding too)
    tr._weight_grads(t, tr._scratch(6144)[1], 6144)
    assert torch.equal(first, tr._flat_grads)
    pad = _padding(*tr._layout)
    assert int(pad.sum()) > 0 and (first[pad] == 0.0).all() and first[~pad].abs().max().item() > 0.0


def test_every_grad_is_a_view_of_the_flat_tensor():
    from rl_collision_avoidance_amd import _lib
    net = build_net(WS, 3, seed=25).cuda()
    tr = _trainer(net, learning_rate=0.0)
    x, y, a = _batch(net, 64, seed=7)
    tr.train(x, y, a)
    off, size, total = _lib.policy_param_layout_ws(3, 11)
    assert tr._flat_grads.numel() == total
    for name, o, n in zip(_lib.POLICY_PARAM_NAMES_WS, off, size):
        g = getattr(net, name).grad
        assert g._base is tr._flat_grads and g.data_ptr() == tr._flat_grads.data_ptr() + 4 * o, name
        assert g.shape == getattr(net, name).shape and g.numel() == n and g.is_contiguous(), name
    # a caller's optimiser works on them (train_regression(opt=...))
    sgd = torch.optim.SGD(net.parameters(), lr=0.1)
    before = net.fc1_kernel.detach().clone()
    tr.train_regression(x, y, a, opt=sgd)
    moved = before - 0.1 * net.fc1_kernel.grad
    assert (net.fc1_kernel.detach() - moved).abs().max().item() <= 4 * U * moved.abs().max().item() < (moved - before).abs().max().item()


# ---- the optimiser in isolation ---------------------------------------------------------------------------------------------------
CLIP = 0.01
KINDS = {"adam": ("adam", dict(beta1=0.9, beta2=0.999, eps=1e-8)), "rmsprop": ("rmsprop", dict(decay=0.99, momentum=0.0, eps=0.1)),
         "rmsprop-momentum": ("rmsprop", dict(decay=0.99, momentum=0.9, eps=0.1))}
LRS = [1e-3, 3e-4, 2e-3, 5e-5]


class _Apply(object):
    """random masters (twelve allocations of their own) and state in the weight-sharing layout on a handle, stepped by the raw cavoid_policy_apply_ws"""

    def __init__(self, A, kind, hyper, clip, seed):
        from rl_collision_avoidance_amd import _lib
        from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
        self.names, self.lib = _lib.POLICY_PARAM_NAMES_WS, _lib.lib()
        self.net = build_net(WS, 3, seed=seed, A=A).cuda()
        self.pol = FusedPolicy(self.net)
        self.off, self.size, self.total = _lib.policy_param_layout_ws(3, A)
        g = torch.Generator().manual_seed(seed)
        self.shapes = [tuple(getattr(self.net, n).shape) for n in self.names]
        self.masters = [(torch.randn(s, generator=g) * 0.2).cuda() for s in self.shapes]
        self.w = self.pol.weights_struct(with_backward=True)
        for name, m in zip(self.names[2:], self.masters[2:]):      # (other_kernel / other_bias are arguments of their own)
            setattr(self.w, name, _ptr(m))
        self.state1 = torch.zeros(self.total, device="cuda")
        self.state2 = torch.zeros(self.total, device="cuda")
        if kind == "rmsprop":
            for v in self.split(self.state1):
                v.fill_(1.0)
        self.step = torch.zeros(1, dtype=torch.int64, device="cuda")
        o = _lib.CavoidPolicyOptimizer()
        o.struct_size, o.kind = C.sizeof(o), (_lib.OPT_RMSPROP if kind == "rmsprop" else _lib.OPT_ADAM)
        o.decay1, o.decay2 = (hyper["decay"], hyper["momentum"]) if kind == "rmsprop" else (hyper["beta1"], hyper["beta2"])
        o.eps, o.clip_average_norm = hyper["eps"], (clip or 0.0)
        o.state1, o.state2, o.step = _ptr(self.state1), _ptr(self.state2), _ptr(self.step)
        self.o = o

    def split(self, flat):
        return [flat[o:o + n].view(s) for o, n, s in zip(self.off, self.size, self.shapes)]

    def grads(self, seed, boost=None):
        """a flat gradient vector (zero padding); `boost` = (index, factor) scales one variable's gradient"""
        g = torch.Generator().manual_seed(seed)
        flat = torch.zeros(self.total)
        for i, (o, n) in enumerate(zip(self.off, self.size)):
            flat[o:o + n] = torch.randn(n, generator=g) * (boost[1] if boost and boost[0] == i else 1.0)
        return flat.cuda()

    def call(self, h, w, ok, ob, o, flat):
        return self.lib.cavoid_policy_apply_ws(h, w, ok, ob, o, flat, self.pol._stream())

    def apply(self, flat, lr):
        self.o.lr = lr
        return self.call(self.pol._h, C.byref(self.w), _ptr(self.masters[0]), _ptr(self.masters[1]), C.byref(self.o), _ptr(flat))


@pytest.mark.parametrize("clip", [None, CLIP], ids=["noclip", "clip"])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("A", [11, 5])
def test_apply_ws_is_the_update_rule(A, kind, clip):
    """the body and bound of test_apply_is_the_update_rule on the weight-sharing layout: four steps, another lr each: masters and both
    state vectors against the float64 rule, within max(3 x the error of the same rule in float32 torch tensor ops on the same inputs,
    2^-22 of the tensor's largest entry)"""
    name, hyper = KINDS[kind]
    ap = _Apply(A, name, hyper, clip, seed=60 + A)
    w0 = [m.clone() for m in ap.masters]
    big, small = 4, 6                                      # layer2_kernel's gradient is scaled up, fullyconnected1's is not
    flats = [ap.grads(70 + t, boost=(big, 10.0)) for t in range(4)]
    per_step = [ap.split(f) for f in flats]
    if clip is not None:                                   # the inputs put one variable above the clip and one below it, every step
        for gs in per_step:
            assert rules.average_norm(gs[big]) > clip > rules.average_norm(gs[small])
    for t, lr in enumerate(LRS):
        kept = flats[t].clone()
        assert ap.apply(flats[t], lr) == 0
        assert int(ap.step.item()) == t + 1
        assert torch.equal(flats[t], kept)                 # the clip scales what the update reads, not grads_flat
    want = rules.run_steps(name, w0, per_step, LRS, clip=clip, dtype=torch.float64, **hyper)
    f32 = rules.run_steps(name, w0, per_step, LRS, clip=clip, dtype=torch.float32, **hyper)
    got = (ap.masters, ap.split(ap.state1), ap.split(ap.state2))
    worst = 0.0
    for what, g_, w_, f_ in zip(("master", "state1", "state2"), got, want, f32):
        for i, pname in enumerate(ap.names):
            err = (g_[i].double() - w_[i]).abs().max().item()
            err32 = (f_[i].double() - w_[i]).abs().max().item()
            bound = max(3.0 * err32, 2.0 ** -22 * w_[i].abs().max().item())
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else float("inf")))
            assert err <= bound, (what, pname, err, err32, bound)
    print("largest error / bound: %.3f" % worst)
    pad = _padding(ap.off, ap.size, ap.total)
    assert (ap.state1[pad] == 0).all() and (ap.state2[pad] == 0).all()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_apply_ws_with_lr_zero_leaves_the_masters_alone(kind):
    name, hyper = KINDS[kind]
    ap = _Apply(11, name, hyper, CLIP, seed=80)
    w0 = [m.clone() for m in ap.masters]
    assert ap.apply(ap.grads(81), 0.0) == 0
    for m, b in zip(ap.masters, w0):
        assert torch.equal(m, b)
    assert int(ap.step.item()) == 1 and ap.state1.abs().max().item() > 0.0


# ---- the re-pack ------------------------------------------------------------------------------------------------------------------
def _assert_handle_follows_the_masters(tr, net, seed):
    """forward on 200 rows and trainer passes: the stepped handle against a fresh load of the updated module, bit for bit.
    `loss` is summed with one float atomic per WAVEFRONT of the forward kernel (16 rows each), in arrival order: two identical calls on
    one handle may differ in its last bit as soon as two wavefronts hold rows (tests/test_gpu_policy_step.py).  So gh is compared on 64
    rows, and gh AND loss on 16 rows, where one wavefront adds the rows' costs and the others add 0.0: the sum then has one order."""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer, FusedPolicy
    x, y, a = _batch(net, 200, seed=seed)
    p, v = tr.policy(x)
    fresh = FusedPolicy(net, ws_crowd=tr.ws_crowd)
    p2, v2 = fresh(x)
    assert torch.equal(p, p2) and torch.equal(v, v2)
    other = FusedA3CTrainer(net, policy=fresh, learning_rate=0.0)          # (refreshes `fresh` with_backward = 1: a fresh load)
    for rows in (64, 16):
        args = (x[:rows].contiguous(), y[:rows].contiguous(), a[:rows].to(torch.int32), rows)
        t1 = tr._pass(*args)
        gh, loss = t1["gh"].clone(), t1["loss"].clone()
        t2 = other._pass(*args)
        assert torch.equal(gh, t2["gh"]) and gh.abs().max().item() > 0.0, rows
        assert (loss - t2["loss"]).abs().max().item() <= 8 * U * loss.abs().max().item() and loss.abs().min().item() > 0.0, rows
        if rows == 16:
            assert torch.equal(loss, t2["loss"])


@pytest.mark.parametrize("M", [3, 20])
def test_after_apply_ws_the_handle_is_a_fresh_load_of_the_masters(M):
    net = build_net(WS, M, seed=26).cuda()
    before = {k: net.get_parameter(k).detach().clone() for k in ("fc1_kernel", "other_kernel")}
    tr = _trainer(net, learning_rate=1e-3)
    x, y, a = _batch(net, 200, seed=8)
    tr.train(x, y, a)
    for k, b in before.items():                            # the step moved the module's own storage
        assert (net.get_parameter(k).detach() - b).abs().max().item() > 1e-4, k
    _assert_handle_follows_the_masters(tr, net, seed=9)


def test_ws_device_step_learns_like_the_existing_trainer():
    """the body and the two bounds of test_device_step_learns_like_the_existing_trainer, FusedA3CTrainer against
    FusedA3CTrainer(ws_device_step=True): five steps of 4096 rows at M = 7"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    net_a = build_net(WS, 7, seed=31).cuda()
    net_b = copy.deepcopy(net_a)
    ta, tb = FusedA3CTrainer(net_a, learning_rate=1e-4), FusedA3CTrainer(net_b, learning_rate=1e-4, ws_device_step=True)
    for step in range(5):
        x = inputs(net_a, 4096, seed=100 + step)
        g = torch.Generator().manual_seed(step)
        y = torch.randn(4096, generator=g).cuda()
        a = torch.randint(0, 11, (4096,), generator=g).cuda()
        la = float(ta.train(x, y, a))
        lb = float(tb.train(x, y, a))
        assert abs(la - lb) <= 1e-3 * max(1.0, abs(la))
    for (k, pa), (_, pb) in zip(net_a.named_parameters(), net_b.named_parameters()):
        assert (pa - pb).abs().max().item() <= 2e-5, k
    assert ta.training_step == tb.training_step == 5 and int(tb.opt.step_count.item()) == 5


def test_ws_device_step_accepts_an_empty_batch():
    net = build_net(WS, 3, seed=41).cuda()
    tr = _trainer(net)
    x, y, a = _batch(net, 128, seed=5)
    loss = tr.train(x[:0], y[:0], a[:0])
    assert float(loss) == 0.0 and tr.training_step == 1 and int(tr.opt.step_count.item()) == 1
    assert (tr._flat_grads == 0).all()
    _assert_handle_follows_the_masters(tr, net, seed=10)


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------
def _stepped(ws_device_step, **kw):
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    net = build_net(WS, 3, seed=51).cuda()
    tr = FusedA3CTrainer(net, learning_rate=1e-3, ws_device_step=ws_device_step, **kw)
    for step in range(3):
        tr.train(*_batch(net, 64, seed=200 + step))
    return net, tr


def _adam_state(tr):
    """{name: (exp_avg, exp_avg_sq, step)} of either trainer tail"""
    if tr.device_step:
        m, v, n = tr._views(tr.opt.state1), tr._views(tr.opt.state2), float(tr.opt.step_count.item())
        return {k: (m[k], v[k], n) for k in m}
    return {k: (tr.opt.state[p]["exp_avg"], tr.opt.state[p]["exp_avg_sq"], float(tr.opt.state[p]["step"])) for k, p in tr.net.named_parameters()}


@pytest.mark.parametrize("saved_with", [True, False], ids=["saved-with-ws-device-step", "saved-without"])
def test_adam_checkpoints_resume_with_and_without_the_ws_device_step(saved_with, tmp_path):
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    from rl_collision_avoidance_amd.ga3c.train import load_checkpoint, save_checkpoint
    net, tr = _stepped(saved_with)
    path = save_checkpoint(str(tmp_path), 7, net, tr)
    entry = torch.load(path, map_location="cuda")["optimizer"]
    assert set(entry) == {"state", "param_groups"} and set(entry["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}    # torch.optim.Adam's format
    want = _adam_state(tr)
    assert set(want) == {k for k, _ in net.named_parameters()}
    for ws_device_step in (False, True):
        net2 = build_net(WS, 3, seed=52).cuda()
        tr2 = FusedA3CTrainer(net2, learning_rate=1e-3, ws_device_step=ws_device_step)
        assert load_checkpoint(path, net2, tr2, torch.device("cuda")) == 7
        got = _adam_state(tr2)
        for k in want:
            assert torch.equal(got[k][0], want[k][0]) and torch.equal(got[k][1], want[k][1]) and got[k][2] == want[k][2] == 3.0, (k, ws_device_step)
        assert torch.equal(net2.other_kernel, net.other_kernel) and tr2.training_step == 3


def test_an_rmsprop_checkpoint_does_not_load_into_an_adam_run_or_the_reverse(tmp_path):
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    from rl_collision_avoidance_amd.ga3c.train import load_checkpoint, save_checkpoint
    net, tr = _stepped(True, optimizer="rmsprop", grad_clip=40.0)
    path = save_checkpoint(str(tmp_path / "r"), 1, net, tr)
    assert torch.load(path, map_location="cuda")["optimizer"]["kind"] == "rmsprop"
    for ws_device_step in (False, True):
        net2 = build_net(WS, 3, seed=52).cuda()
        with pytest.raises(SystemExit) as e:
            load_checkpoint(path, net2, FusedA3CTrainer(net2, ws_device_step=ws_device_step), torch.device("cuda"))
        assert "rmsprop" in str(e.value) and "adam" in str(e.value)
    net3 = build_net(WS, 3, seed=53).cuda()
    tr3 = FusedA3CTrainer(net3, ws_device_step=True, optimizer="rmsprop")
    load_checkpoint(path, net3, tr3, torch.device("cuda"))
    assert torch.equal(tr3.opt.state1, tr.opt.state1) and torch.equal(tr3.opt.state2, tr.opt.state2) and int(tr3.opt.step_count.item()) == 3
    adam_path = save_checkpoint(str(tmp_path / "a"), 1, *_stepped(False))
    with pytest.raises(SystemExit) as e:
        load_checkpoint(adam_path, net3, tr3, torch.device("cuda"))
    assert "rmsprop" in str(e.value) and "adam" in str(e.value)


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_errors_are_codes_and_value_errors():
    from rl_collision_avoidance_amd import _lib
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer, FusedPolicy
    lib = _lib.lib()
    net = build_net(WS, 3, seed=27).cuda()
    tr = _trainer(net, learning_rate=0.0)
    pol = tr.policy
    x, y, a = _batch(net, 64, seed=11)
    tr.train(x, y, a)
    t, cbuf = tr._scratch(64)
    floats = C.c_int64()
    assert lib.cavoid_policy_weight_grads_scratch_ws(pol._h, 64, C.byref(floats)) == 0
    scratch, flat = torch.empty(floats.value, device="cuda"), tr._flat_grads
    grads = lambda h, b, s, n, f: lib.cavoid_policy_weight_grads_ws(h, b, s, n, f, pol._stream())
    assert grads(pol._h, C.byref(cbuf), _ptr(scratch), floats.value, _ptr(flat)) == 0
    assert grads(pol._h, C.byref(cbuf), _ptr(scratch), floats.value - 1, _ptr(flat)) == EINVAL        # a scratch one float short
    assert grads(pol._h, C.byref(cbuf), None, floats.value, _ptr(flat)) == EINVAL
    assert grads(pol._h, C.byref(cbuf), _ptr(scratch), floats.value, None) == EINVAL
    assert grads(pol._h, None, _ptr(scratch), floats.value, _ptr(flat)) == EINVAL
    assert grads(None, C.byref(cbuf), _ptr(scratch), floats.value, _ptr(flat)) == EINVAL
    assert grads(pol._h, C.byref(cbuf), C.c_void_p(scratch.data_ptr() + 4), floats.value, _ptr(flat)) == EINVAL      # misaligned
    bad = _clone(cbuf)
    bad.struct_size = 8
    assert grads(pol._h, C.byref(bad), _ptr(scratch), floats.value, _ptr(flat)) == EINVAL
    bad = _clone(cbuf)
    bad.gf = None
    assert grads(pol._h, C.byref(bad), _ptr(scratch), floats.value, _ptr(flat)) == EINVAL
    bad = _clone(cbuf)
    bad.capacity_rows = 100                                # not a multiple of 64
    assert grads(pol._h, C.byref(bad), _ptr(scratch), floats.value, _ptr(flat)) == EINVAL
    assert lib.cavoid_policy_weight_grads_scratch_ws(pol._h, 100, C.byref(floats)) == EINVAL
    assert lib.cavoid_policy_weight_grads_scratch_ws(pol._h, 0, C.byref(floats)) == EINVAL
    assert lib.cavoid_policy_weight_grads_scratch_ws(pol._h, 64, None) == EINVAL
    assert lib.cavoid_policy_weight_grads_scratch_ws(None, 64, C.byref(floats)) == EINVAL
    ap = _Apply(11, "adam", KINDS["adam"][1], None, seed=82)
    g, ok, ob, h = ap.grads(83), _ptr(ap.masters[0]), _ptr(ap.masters[1]), ap.pol._h
    assert ap.call(h, None, ok, ob, C.byref(ap.o), _ptr(g)) == EINVAL and ap.call(h, C.byref(ap.w), ok, ob, None, _ptr(g)) == EINVAL
    assert ap.call(h, C.byref(ap.w), ok, ob, C.byref(ap.o), None) == EINVAL and ap.call(None, C.byref(ap.w), ok, ob, C.byref(ap.o), _ptr(g)) == EINVAL
    assert ap.call(h, C.byref(ap.w), None, ob, C.byref(ap.o), _ptr(g)) == EINVAL and ap.call(h, C.byref(ap.w), ok, None, C.byref(ap.o), _ptr(g)) == EINVAL
    for field, value in (("struct_size", 8), ("kind", 2), ("state1", None), ("step", None), ("clip_average_norm", -1.0)):
        o = _clone(ap.o)
        setattr(o, field, value)
        assert ap.call(h, C.byref(ap.w), ok, ob, C.byref(o), _ptr(g)) == EINVAL, field
    w = _clone(ap.w)
    w.struct_size = 8
    assert ap.call(h, C.byref(w), ok, ob, C.byref(ap.o), _ptr(g)) == EINVAL
    w = _clone(ap.w)
    w.p_bias = None
    assert ap.call(h, C.byref(w), ok, ob, C.byref(ap.o), _ptr(g)) == EINVAL
    assert int(ap.step.item()) == 0                        # none of the refused calls stepped
    # an LSTM handle: the _ws device calls are codes, the trainer says so in words
    rnn_net = build_net("rnn", 3, seed=28).cuda()
    rnn = FusedPolicy(rnn_net)
    assert grads(rnn._h, C.byref(cbuf), _ptr(scratch), floats.value, _ptr(flat)) == EUNSUPPORTED
    assert ap.call(rnn._h, C.byref(ap.w), ok, ob, C.byref(ap.o), _ptr(g)) == EUNSUPPORTED
    assert lib.cavoid_policy_weight_grads_scratch_ws(rnn._h, 64, C.byref(floats)) == EUNSUPPORTED
    assert int(ap.step.item()) == 0
    with pytest.raises(ValueError, match="rnn"):
        FusedA3CTrainer(rnn_net, ws_device_step=True)
    with pytest.raises(ValueError, match="ws_device_step"):
        FusedA3CTrainer(net, device_step=True)             # (still refused, and the message names the keyword that works)
    with pytest.raises(ValueError, match="device_step"):
        FusedA3CTrainer(net, optimizer="rmsprop")
    with pytest.raises(ValueError, match="device_step"):
        FusedA3CTrainer(net, grad_clip=40.0)


# ---- the user's path ----------------------------------------------------------------------------------------------------------------
def test_train_cli_with_the_ws_device_step(tmp_path):
    ck = tmp_path / "ck"
    cmd = [sys.executable, "-m", "rl_collision_avoidance_amd.ga3c.train", "--arch", "weight_sharing", "--worlds", "64", "--episodes", "200",
           "--ws-device-step", "--optimizer", "rmsprop", "--grad-clip", "40", "--checkpoint-dir", str(ck), "--print-every", "100"]
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    run = subprocess.run(cmd, cwd=ROOT, env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-3000:])
    assert run.returncode == 0
    assert "trainer tail: cavoid_policy_weight_grads_ws + cavoid_policy_apply_ws (rmsprop, clip_by_average_norm 40) inside the HIP library" in run.stdout
    assert "finished" in run.stdout and " 0 training steps" not in run.stdout
    saved = sorted(os.listdir(str(ck)))
    assert saved
    assert torch.load(str(ck / saved[-1]), map_location="cpu")["optimizer"]["kind"] == "rmsprop"
