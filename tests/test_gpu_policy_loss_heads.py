"""The epilogue that follows the heads -- softmax + MIN_POLICY, the A3C loss and its gradient at the logits, the action draw -- where the
entropy term and the log clamp matter.  It exists in several copies (policy_heads of cavoid_policy.hpp, which the LSTM and the
weight-sharing float32-MFMA kernels share, the softmax blocks of the split / oct forms, split_select_action inlined into the split, oct, pipe, crowd and fused
actor kernels), and the other test files hold all of them to the PyTorch network in ONE regime: fresh Glorot weights, whose softmax is
nearly uniform (no p within four orders of magnitude of LOG_EPSILON, beta = 1e-4: an entropy gradient below the tolerances).  Here:
  * both FusedA3CTrainer paths against float64 autograd of NetworkVP_rnn.loss under test_fused_trainer_gradients_match_autograd's own
    criteria (tests/policy_regimes.py holds the one copy), with beta up to 1, LOG_EPSILON = 0.08 (the clamp cuts through every row) and a
    confident network (p head x 40: most probabilities far below LOG_EPSILON);
  * inference of the float32-grade forms on the confident network against float64, relative to PyTorch's own float32 error;
  * the action draw where over half of the float32 probabilities are exactly 0 (p head x 150): long flat runs in the CDF;
  * the other tile-to-wavefront forms and the fused actor kernel, bit for bit, on such rows.
tests/test_policy_regimes_host.py holds the cases to their conditions on the CPU and shows what a wrong epilogue would do to them."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle.cavoid_oracle import philox4x32
from tests import policy_regimes as R
from tests.policy_support import P_TOL, _check_forms_bit_identical

pytestmark = pytest.mark.gpu


# ---- the trainer epilogues ------------------------------------------------------------------------------------------------------------
def _train_and_check(case, net, x, y, a, tr):
    total, cost_p, cost_v, want, torch32 = R.reference_gradients(net, x, y, a)
    loss = float(tr.train(x, y, a))
    report = []
    try:
        R.assert_loss_matches(loss, total)
        R.assert_gradients_match(net, want, torch32, case.B, report)
    finally:
        print("%s beta=%g: loss %.6e (float64 %.6e: cost_p %.4e cost_v %.4e)" % (R.case_id(case), net.beta, loss, total, cost_p, cost_v))
        for k, err, err32, scale in report:
            print("    %-14s err %.2e  err32 %.2e  scale %.2e  err/scale %.1e" % (k, err, err32, scale, err / scale))
    return want


@pytest.mark.parametrize("case", R.TRAINER_CASES + R.WS_MIN_POLICY_CASES, ids=R.case_id)
def test_trainer_epilogue_matches_float64_autograd(case):
    """cavoid_policy_train / cavoid_policy_train_ws, learning rate 0, on the rows build_case keeps (clear of the clamp threshold)"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    net, x, y, a, info = R.build_case(case, "cuda")
    R.assert_conditions(case, info)
    tr = FusedA3CTrainer(net, learning_rate=0.0)
    assert tr.ws == (case.arch == "weight_sharing")
    _train_and_check(case, net, x, y, a, tr)


@pytest.mark.parametrize("case", R.BETA_SWITCH_CASES, ids=R.case_id)
def test_beta_is_read_at_every_train_call(case):
    """one trainer, the same batch twice, beta = 0 then beta = 1 (ga3c.train's schedule rewrites net.beta every step): each call's
    gradients are the reference's for its own beta"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    net, x, y, a, info = R.build_case(case, "cuda")
    R.assert_conditions(case, info)
    tr = FusedA3CTrainer(net, learning_rate=0.0)
    wants = []
    for beta in (0.0, 1.0):
        net.beta = beta
        wants.append(_train_and_check(case, net, x, y, a, tr))
    d = (wants[0]["p_kernel"] - wants[1]["p_kernel"]).abs().max().item()
    assert d > 1e-2 * wants[0]["p_kernel"].abs().max().item()        # (the two references really differ)


@pytest.mark.parametrize("arch,M", [("rnn", 9), ("weight_sharing", 7)])
def test_trainer_writes_every_scratch_row_it_lets_the_gemms_read(arch, M):
    """include/cavoid.h: every per-row buffer is written by each call, the weight-gradient GEMMs may run over all capacity_rows.  The
    scratch is filled with NaN first (0 x NaN is NaN), the batch ends inside a 2048-row slice and holds a tile whose rows all stop
    after one LSTM step: policy_forward_kernel<4, true> writes h_in[t] only for the steps some row of the tile takes, and
    d lstm = sum_t h_in[t]^T gl[t] ran over what the allocator had left there (found as a NaN lstm_kernel gradient at M = 9,
    B = 1000, once an earlier test had left NaNs in freed memory)."""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer
    B = 2100
    case = R.Case("beta", arch, M, B, 1e-4, 1e-6, 0.0, 0.0, False, 11)
    net = R.build_net(arch, M, seed=20 + M).cuda()
    x = R.inputs(net, 3200, seed=B + 1)
    x = x[R.clear_of_relu_kinks(net, x)]
    short = x[:, 0] <= 1.0
    x = torch.cat([x[~short][:64], x[short][:64], x[~short][64:]])[:B]          # rows 64 .. 127: one tile of rows that stop early
    assert x.shape[0] == B and float(x[64:128, 0].max()) == 1.0 and float(x[:, 0].max()) == M
    g = torch.Generator().manual_seed(B)
    y, a = torch.randn(B, generator=g).cuda(), torch.randint(0, 11, (B,), generator=g).cuda()
    tr = FusedA3CTrainer(net, learning_rate=0.0)
    buffers, _ = tr._scratch(4096)                           # (train's own row count for 2100 rows)
    for t in buffers.values():
        t.fill_(float("nan"))
    _train_and_check(case, net, x, y, a, tr)
    assert tr._scratch(4096)[0] is buffers and len(tr._buffers) == 1


@pytest.mark.parametrize("A", [5, 15])
def test_ws_other_action_counts(A):
    """test_other_action_counts for the weight-sharing handle: heads of 5 and 15 logits through its own inference kernel, action draw
    and trainer pass"""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedA3CTrainer, FusedPolicy
    net = R.build_net("weight_sharing", 7, seed=80 + A, A=A).cuda()
    B = 777
    x = R.inputs(net, B, seed=A)
    pol = FusedPolicy(net, seed=5)
    a_s, p, v = pol.act(x)
    with torch.no_grad():
        _, p_ref, v_ref = net.forward(x)
    assert p.shape == (B, A) and (p - p_ref).abs().max().item() <= P_TOL and int(a_s.max()) < A and int(a_s.min()) >= 0
    g = torch.Generator().manual_seed(A)
    y = torch.randn(B, generator=g).cuda()
    a = torch.randint(0, A, (B,), generator=g).cuda()
    net.zero_grad()
    net.loss(x, y, torch.nn.functional.one_hot(a, A).float())[0].backward()
    want = {k: t.grad.clone() for k, t in net.named_parameters()}
    FusedA3CTrainer(net, pol, learning_rate=0.0).train(x, y, a)
    for k, t in net.named_parameters():
        scale = want[k].abs().max().item() + 1e-6
        assert (t.grad - want[k]).abs().max().item() <= 2e-4 * scale, k


# ---- inference and the action draw on confident networks ---------------------------------------------------------------------------
FORMS = {"default": ("0", ("split", 16)), "f32": ("1", ("f32", 0)), "crowd": ("0", ("split", 16)), "weight_sharing": ("0", ("f32", 0))}


def _confident_policy(form, gain, monkeypatch, seed=0):
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    f32, inference_form = FORMS[form]
    monkeypatch.setenv("CAVOID_POLICY_F32", f32)
    monkeypatch.setenv("CAVOID_POLICY_PRODUCTS", "16")
    net = R.form_net(form, gain).cuda()
    pol = FusedPolicy(net, seed=seed)
    assert pol.inference_form == inference_form and pol.crowd == (form == "crowd") and pol.ws == (form == "weight_sharing")
    return net, pol


@pytest.mark.parametrize("form", list(FORMS))
def test_float32_grade_forms_on_a_confident_network(form, monkeypatch):
    """p head x 40, 4096 rows, against the float64 network.  An absolute bar on p says nothing here (an honest logit error of 1e-4 is
    2.5e-5 in a p near 0.5, and anything passes at p = 1e-20), so: max |p - p64|, max |v - v64| and max |log p - log p64| (where
    p64 >= 1e-30) within 6x of what PyTorch's float32 forward differs from float64 by (+ the floors, and the factor, of
    test_both_inference_kernels_against_a_float64_yardstick)."""
    net, pol = _confident_policy(form, R.GAIN_TRAINER, monkeypatch)
    x = R.inputs(net, R.ACCURACY_ROWS, seed=7)
    p, v = pol(x)
    with torch.no_grad():
        _, p32, v32 = net.forward(x)
    p64, v64 = R.forward64(net, x)
    assert torch.isfinite(p).all() and torch.isfinite(v).all() and (p >= 0).all()
    assert (p.sum(dim=1) - 1.0).abs().max().item() <= 1e-5
    seen = p64 >= 1e-30
    assert (p64 <= 1e-6).float().mean().item() >= 0.5 and seen.float().mean().item() >= 0.5      # (conditions: confident, and measurable)

    def errors(pp, vv):
        e_log = (torch.log(pp.double()) - torch.log(p64))[seen].abs().max().item()
        return (pp.double() - p64).abs().max().item(), (vv.double() - v64).abs().max().item(), e_log
    e_p, e_v, e_log = errors(p, v)
    e_torch_p, e_torch_v, e_torch_log = errors(p32, v32)
    print("confident policy kernel %s M=%d gain=%g: |dp| %.2e (torch f32 %.2e)  |dv| %.2e (torch f32 %.2e)  |dlog p| %.2e (torch f32 %.2e)"
          % (form, net.max_others, R.GAIN_TRAINER, e_p, e_torch_p, e_v, e_torch_v, e_log, e_torch_log))
    info = (form, e_p, e_torch_p, e_v, e_torch_v, e_log, e_torch_log)
    assert e_p <= 6.0 * e_torch_p + 5e-8 and e_v <= 6.0 * e_torch_v + 5e-7, info
    assert e_log <= 6.0 * e_torch_log, info


@pytest.mark.parametrize("form", list(FORMS))
def test_action_draw_where_most_probabilities_are_zero(form, monkeypatch):
    """p head x 150: over half of the float32 probabilities are exactly 0, so the CDF has long flat runs -- where `cdf <= u * total`,
    the clamp to A - 1 and the greedy 'first index of the maximum' can go wrong unseen on near-uniform rows."""
    SEED = 0x1234567890AB
    net, pol = _confident_policy(form, R.GAIN_DRAW, monkeypatch, seed=SEED)
    B, A = R.DRAW_ROWS, 11
    x = R.inputs(net, B, seed=8)
    a_g, p, _ = pol.act(x, greedy=True)
    pn = p.cpu().numpy()
    assert (pn == 0.0).mean() >= 0.5                         # (condition: the reason for this gain)
    assert np.array_equal(a_g.cpu().numpy(), np.argmax(pn, axis=1))          # numpy: the first index of the maximum
    draws = []
    for _ in range(3):
        a, p_k, _ = pol.act(x)
        assert torch.equal(p_k, p)
        draws.append(a.cpu().numpy())
    cdf = np.cumsum(pn.astype(np.float64), axis=1)
    for k, a in enumerate(draws):
        assert a.min() >= 0 and a.max() < A
        assert (pn[np.arange(B), a] > 0.0).all(), (form, k, int((pn[np.arange(B), a] <= 0.0).sum()))     # no exceptions
        step, bad = 1 + k, 0                                 # every launch that selects actions advances the counter: greedy was 0
        for row in range(0, B, 7):
            bits = philox4x32(row, 0, step, 0x504F4C, SEED & 0xFFFFFFFF, SEED >> 32)[0]
            u = (bits >> 8) / 16777216.0
            expect = min(int(np.sum(cdf[row] <= u * cdf[row, -1])), A - 1)
            if expect != a[row]:
                # only a draw within float32 rounding of a CDF boundary may land on the neighbour
                assert np.min(np.abs(cdf[row] - u * cdf[row, -1])) < 1e-6, (form, row, step, expect, a[row])
                bad += 1
        assert bad <= 2, (form, k, bad)
    assert not np.array_equal(draws[0], draws[1])


@pytest.mark.parametrize("form", ["oct", "duo", "pipe"])
def test_other_tile_to_wavefront_forms_are_bit_identical_on_a_confident_network(form, monkeypatch):
    """test_other_tile_to_wavefront_forms_are_bit_identical's body on the p head x 150"""
    M, B = 3, 5000
    net = R.confident(R.build_net("rnn", M, seed=60 + M), R.GAIN_DRAW).cuda()
    x = R.inputs(net, B, seed=11)
    p4 = _check_forms_bit_identical(net, x, M, B, form, monkeypatch)
    assert (p4 == 0.0).float().mean().item() >= 0.5


def test_fused_actor_equals_step_by_step_on_a_confident_network():
    """The actor kernel inlines the same split_select_action next to its env step; test_fused_actor_equals_step_by_step only ever
    feeds it near-uniform rows.  Its networks have zero biases, hence the larger gain (p_kernel x 1000)."""
    from rl_collision_avoidance_amd.ga3c.policy_kernel import FusedPolicy
    from tests.actor_twins import make, same as _same
    W, N = 512, 4
    env_a, net_a, pol_a, a = make(W, N, None, 21)              # (tests/test_gpu_actor.py's twins)
    env_b, net_b, pol_b, b = make(W, N, None, 21)
    for net, pol in ((net_a, pol_a), (net_b, pol_b)):
        with torch.no_grad():
            net.p_kernel.mul_(R.GAIN_ACTOR)
        pol.refresh()
    assert a.fused_available and a.actor_path.startswith("fused actor kernel"), a.actor_path
    for p, q in zip(net_a.parameters(), net_b.parameters()):
        assert torch.equal(p, q)
    _same(a.obs, b.obs, "first observation")
    p0, _ = FusedPolicy(net_a)(a.obs.view(W * N, -1)[:, 1:])
    assert (p0 == 0.0).float().mean().item() >= 0.25
    total = 0
    for k in (2, 1, 7, 16):
        a.run_fused(k)
        for _ in range(k):
            b.step()
        total += k
        _same(a.obs, b.obs, ("obs", total))
        for s, t in zip(env_a.get_state(), env_b.get_state()):
            _same(s, t, ("state", total))
        _same(env_a.episode, env_b.episode, ("episode", total))
        _same(env_a.rewards, env_b.rewards, ("rewards", total))
        _same(env_a.done, env_b.done, ("done", total))
        _same(env_a.game_over, env_b.game_over, ("game_over", total))
        for name in ("x", "val", "ret", "act_ring", "emit_t"):
            _same(getattr(a, name), getattr(b, name), (name, total))
        assert a.step_index == b.step_index == total
    assert len(torch.unique(a.act_ring[:total])) >= 2
    for r in (a, b):
        r.close()
    for e in (env_a, env_b):
        e.close()
