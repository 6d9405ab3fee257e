"""The update rules of ``cavoid_policy_apply`` (include/cavoid.h) restated on torch tensors of any dtype -- float64 as the yardstick
of tests/test_gpu_policy_step.py, float32 for the error a float32 evaluation of the same rule has on the same inputs.  A plain module;
tests/test_policy_step_host.py holds the restatements to something that is not themselves (``torch.optim.Adam`` / ``torch.optim.RMSprop``
on float64 CPU tensors, the clip's closed form).  Every function is out of place: (new w, new state1, new state2)."""
import torch


def clip_by_average_norm(g, c):
    """``tf.clip_by_average_norm(g, c)``: g * c / max(||g||_2 / n, c), n = the tensor's element count."""
    avg = g.norm() / g.numel()
    return g * (c / torch.clamp_min(avg, c))


def average_norm(g):
    return float(g.double().norm() / g.numel())


def adam_step(w, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """``torch.optim.Adam`` (no amsgrad, no weight decay), step number t = 1, 2, ..."""
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * (g * g)
    step_size = lr / (1.0 - beta1 ** t)
    denom = v.sqrt() / (1.0 - beta2 ** t) ** 0.5 + eps
    return w - step_size * (m / denom), m, v


def rmsprop_step(w, g, ms, mom, lr, decay=0.99, momentum=0.0, eps=0.1):
    """``tf.train.RMSPropOptimizer`` (not centred) as TensorFlow publishes it: ms = decay ms + (1 - decay) g^2,
    mom = momentum mom + lr g / sqrt(ms + eps) -- epsilon INSIDE the root --, w -= mom.
    Pinned to ``torch.optim.RMSprop`` only where the two rules coincide (eps = 0, constant lr: tests/test_policy_step_host.py); away from
    that regime -- PyTorch adds eps outside the root and scales the whole momentum buffer by lr -- this is unpinned: a restatement of
    the published rule, TensorFlow itself cannot run here."""
    ms = decay * ms + (1.0 - decay) * (g * g)
    mom = momentum * mom + lr * g / (ms + eps).sqrt()
    return w - mom, ms, mom


def run_steps(kind, w, grads, lrs, clip=None, dtype=torch.float64, **hyper):
    """Apply len(lrs) steps of `kind` ('adam' / 'rmsprop') to the list of tensors `w` with the per-step lists `grads[step]`, every tensor
    evaluated in `dtype`.  Returns (w, state1, state2) as lists of `dtype` tensors.  RMSProp's ms starts at ones, as TensorFlow's."""
    w = [t.to(dtype) for t in w]
    s1 = [torch.ones_like(t) if kind == "rmsprop" else torch.zeros_like(t) for t in w]
    s2 = [torch.zeros_like(t) for t in w]
    for t, lr in enumerate(lrs, start=1):
        for i in range(len(w)):
            g = grads[t - 1][i].to(dtype)
            if clip is not None:
                g = clip_by_average_norm(g, clip)
            if kind == "adam":
                w[i], s1[i], s2[i] = adam_step(w[i], g, s1[i], s2[i], t, lr, **hyper)
            else:
                w[i], s1[i], s2[i] = rmsprop_step(w[i], g, s1[i], s2[i], lr, **hyper)
    return w, s1, s2
