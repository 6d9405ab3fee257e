"""CPU side of tests/test_gpu_policy_loss_heads.py: every case that file runs on the GPU is built here from the same table
(tests/policy_regimes.py) with the float64 network alone, and held to the conditions that make it worth running -- the clamp band
excludes few rows, both sides of LOG_EPSILON are populated among all probabilities and among the selected ones -- so that a later
change of a seed or a helper cannot quietly empty one side of the clamp.  And, with float64 autograd, that in each regime the wrong
epilogue it exists to catch moves some gradient by more than 1e-2 of its largest entry: 100x the 1e-4 the GPU tests allow."""
import pytest

torch = pytest.importorskip("torch")

from tests import policy_regimes as R

CASES = list({R.case_id(c): c for c in R.ALL_CASES}.values())


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_every_gpu_case_meets_its_conditions(case):
    net, x, y, a, info = R.build_case(case)
    assert x.shape == (case.B, net.input_size) and y.shape == a.shape == (case.B,)
    assert net.beta == case.beta and net.log_epsilon == case.log_eps and net.min_policy == case.min_policy
    R.assert_conditions(case, info)
    if case.regime == "confident" and case.min_policy > 0.0:
        # nothing is clamped, most of the probabilities sit at the floor MIN_POLICY / (1 + A MIN_POLICY)
        p, _ = R.forward64(net, x)
        floor = case.min_policy / (1.0 + case.A * case.min_policy)
        assert (p < 1.001 * floor).float().mean().item() >= 0.5
    if case.y_near_v:
        _, v = R.forward64(net, x)
        assert (y.double() - v).abs().max().item() < 0.1


@pytest.mark.parametrize("form", list(R.FORM_NETS))
def test_the_inference_networks_are_confident(form):
    """the conditions of the GPU accuracy and action-draw tests, on PyTorch's own forward pass: at gain 40 most probabilities are
    below 1e-6 and most are still measurable (>= 1e-30); at gain 150 over half of the float32 probabilities are exactly 0"""
    below, seen, zeros = R.confident_shares(form)
    assert below >= 0.5 and seen >= 0.5 and zeros >= 0.5, (form, below, seen, zeros)


def test_no_kept_row_sits_on_a_relu_kink():
    case = [c for c in CASES if c.arch == "weight_sharing" and c.M == 7 and c.B == 8192][0]
    net, x, _, _, info = R.build_case(case)
    assert info["excluded"] > 0.0 and R.relu_inputs64(net, x).abs().min().item() > R.RELU_BAND
    assert R.relu_inputs64(net, x).shape == (case.B, 64 * case.M + 3 * 256)


def _mutation_of(case):
    if case.B != 1000 or case.y_near_v:
        return None
    if case.regime == "wide":
        return "entropy_ignores_clamp" if case.beta == 1.0 else "policy_ignores_clamp"
    if case.regime == "confident" and case.min_policy == 0.0:
        return "policy_ignores_clamp"
    if case.regime == "beta" and case.beta == 1.0:
        return "no_entropy_gradient"
    return None


@pytest.mark.parametrize("case", [c for c in CASES if _mutation_of(c)], ids=R.case_id)
def test_a_wrong_epilogue_would_move_the_gradients(case):
    net, x, y, a, _ = R.build_case(case)
    _, _, _, want, _ = R.reference_gradients(net, x, y, a)
    # the epilogue's formula for d cost / d p, unmutated, is the gradient of NetworkVP_rnn.loss ...
    assert R.largest_move(R.epilogue_gradients(net, x, y, a), want) <= 1e-9
    # ... and with the regime's mutation it is far from it (measured: at least 3.5e-1)
    move = R.largest_move(R.epilogue_gradients(net, x, y, a, _mutation_of(case)), want)
    print("%s: %s moves a gradient by %.2e of its largest entry" % (R.case_id(case), _mutation_of(case), move))
    assert move > 1e-2, (case, move)


def test_default_beta_hides_the_entropy_gradient_and_the_plus_one():
    """why the regimes exist: at beta = 1e-4 and default weights, deleting the entropy gradient stays within a few 1e-4 of the
    gradients' largest entries, and ignoring the clamp in it changes nothing at all (no p is below LOG_EPSILON)"""
    case = R.Case("beta", "rnn", 3, 1000, 1e-4, 1e-6, 0.0, 0.0, False, 11)
    net, x, y, a, info = R.build_case(case)
    assert info["below"] == 0.0
    want = R.epilogue_gradients(net, x, y, a)
    assert R.largest_move(R.epilogue_gradients(net, x, y, a, "no_entropy_gradient"), want) < 1e-3
    assert R.largest_move(R.epilogue_gradients(net, x, y, a, "entropy_ignores_clamp"), want) == 0.0
    assert R.largest_move(R.epilogue_gradients(net, x, y, a, "policy_ignores_clamp"), want) == 0.0
