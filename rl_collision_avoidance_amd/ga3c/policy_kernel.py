"""``FusedPolicy`` -- the actors' ``predict_p_and_v`` (+ ``select_action``) as one MFMA kernel launch.

Host mirror of ``cavoid_policy_*`` (include/cavoid.h): takes a ``NetworkVP_rnn`` (arch 'rnn' or 'weight_sharing'), hands its
parameters to the library in the reference checkpoint's layout, and is then callable like
``NetworkVPCore.predict_p_and_v`` (/root/reference/ga3c/GA3C/NetworkVPCore.py:175-176).  The network module stays
the single owner of the weights (the trainer updates it); call ``refresh()`` after an optimiser step.
There is no fallback: without the HIP library / a GPU this raises."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from .. import _lib
from .network import NetworkVP_rnn, split_k_factor


# the most observed neighbours the fused trainer and the fused actor kernel carry (kPolMaxOthers, cavoid_policy.hpp -- tests/test_crowd_host.py
# holds the two equal): wider rows train through autograd and act step by step
MAX_OTHERS = 19
# ... and fused inference (FusedPolicy: predict_p_and_v + select_action), on the crowd kernel above MAX_OTHERS (kPolMaxOthersInference,
# cavoid_policy_crowd.hpp)
MAX_OTHERS_INFERENCE = 64
# the most observed neighbours the fused trainer carries when asked to (FusedA3CTrainer(crowd=True)): rows above MAX_OTHERS run the ring trainer
# kernels (kPolMaxOthersTrain, cavoid_policy_train_ring.hpp -- tests/test_policy_train_ring_host.py holds the two equal)
MAX_OTHERS_TRAIN = 64
# the most observed neighbours the weight-sharing kernels carry, inference and trainer alike (kWsMaxOthers, cavoid_policy_ws.hpp --
# tests/test_policy_ws_host.py holds the two equal): wider weight-sharing rows act and train through PyTorch
MAX_OTHERS_WS = 19
# ... and when asked to (FusedPolicy(ws_crowd=True), FusedA3CTrainer(ws_crowd=True)): rows above MAX_OTHERS_WS run the weight-sharing ring
# kernels on a cavoid_policy_create_ws_crowd handle (kWsMaxOthersCrowd, cavoid_policy_wsring.hpp -- tests/test_policy_wsring_host.py holds the
# two equal)
MAX_OTHERS_WS_CROWD = 64

class FusedPolicy(object):
    accepts_strided_obs = True          # BatchedRollout hands over the env's obs tensor itself, no slice copy

    def __init__(self, net: NetworkVP_rnn, seed: int = 0, forget_bias: float = 1.0, ws_crowd: bool = False):
        """``ws_crowd=True`` (opt-in) carries a 'weight_sharing' network of MAX_OTHERS_WS + 1 .. MAX_OTHERS_WS_CROWD observed neighbours on the
        ring kernels of cavoid_policy_wsring.hpp; it changes nothing for a narrower one and is ignored for 'rnn'."""
        if net.arch not in ("rnn", "weight_sharing"):
            raise ValueError("FusedPolicy implements MULTI_AGENT_ARCH 'rnn' and 'weight_sharing', not %r" % (net.arch,))
        self.arch = net.arch
        dev = net.layer1_kernel.device
        if dev.type != "cuda":
            raise ValueError("FusedPolicy needs the network on the GPU")
        self.net, self.device = net, dev
        self.num_actions, self.max_others, self.input_size = net.num_actions, net.max_others, net.input_size
        self.forget_bias = float(forget_bias)
        self.ws = self.arch == "weight_sharing"      # the weight-sharing kernels (cavoid_policy_create_ws): float32 MFMA, no split form
        ws_crowd = bool(ws_crowd) and self.ws and MAX_OTHERS_WS < self.max_others <= MAX_OTHERS_WS_CROWD
        if self.ws and self.max_others > MAX_OTHERS_WS and not ws_crowd:
            raise ValueError("FusedPolicy carries the weight_sharing network up to %d observed neighbours (kWsMaxOthers), the network "
                             "observes %d" % (MAX_OTHERS_WS, self.max_others))
        if self.max_others > MAX_OTHERS_INFERENCE:
            raise ValueError("FusedPolicy carries up to %d observed neighbours, the network observes %d" % (MAX_OTHERS_INFERENCE, self.max_others))
        self.crowd = self.max_others > MAX_OTHERS      # the crowd handle: inference in float16 or bf16 pieces, the trainer pass on the ring kernels (include/cavoid.h)
        self._lib = _lib.lib()
        h = C.c_void_p()
        name = "cavoid_policy_create" + ("_ws_crowd" if ws_crowd else "_ws" if self.ws else "")
        _lib.check(getattr(self._lib, name)(self.max_others, self.num_actions, dev.index or 0, C.byref(h)), name)
        self._h = h
        # the inference form is fixed at creation (CAVOID_POLICY_F32 / CAVOID_POLICY_PRODUCTS are read by cavoid_policy_create only)
        use_split, products = C.c_int32(), C.c_int32()
        _lib.check(self._lib.cavoid_policy_info(h, None, C.byref(use_split), C.byref(products), None), "cavoid_policy_info")
        self.inference_form = ("split", int(products.value)) if use_split.value else ("f32", 0)
        self.seed(seed)
        self.refresh(check_range=True)

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h:
            torch.cuda.synchronize(self.device)
            self._lib.cavoid_policy_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def seed(self, seed: int) -> None:
        _lib.check(self._lib.cavoid_policy_seed(self._h, C.c_uint64(int(seed) & (2 ** 64 - 1)), self._stream()), "cavoid_policy_seed")

    def clamped_weights(self) -> int:
        """How many weights of the last ``refresh`` the default float16-split form had to clamp to +-65504 (include/cavoid.h,
        cavoid_policy_info; always 0 for the bf16 / float32 forms).  Synchronises the current stream."""
        n = C.c_int32()
        _lib.check(self._lib.cavoid_policy_info(self._h, self._stream(), None, None, C.byref(n)), "cavoid_policy_info")
        return int(n.value)

    def refresh(self, with_backward: bool = False, check_range: bool = False) -> None:
        """Re-pack the module's current parameters (after a trainer step / checkpoint load).  ``with_backward`` also
        packs the transposed copies the fused trainer pass needs.  ``check_range`` (the constructor and checkpoint loads use it; it
        costs a stream synchronisation): fail loudly when a weight lies beyond the float16 split's +-65504 instead of running a
        network that silently differs from the reference's float32 predictor."""
        n = self.net
        w = self.weights_struct(with_backward)
        ptr = lambda t: C.c_void_p(self._f32(t).data_ptr())
        if self.ws:
            _lib.check(self._lib.cavoid_policy_load_ws(self._h, C.byref(w), ptr(n.other_kernel), ptr(n.other_bias), self._stream()),
                       "cavoid_policy_load_ws")
            return
        _lib.check(self._lib.cavoid_policy_load(self._h, C.byref(w), self._stream()), "cavoid_policy_load")
        if check_range and self.inference_form == ("split", 16):
            bad = self.clamped_weights()
            if bad:
                escape = ("CAVOID_POLICY_PRODUCTS=3 (bf16 pieces, float32's range; the one other form above %d observed neighbours)" % MAX_OTHERS
                          if self.crowd else "CAVOID_POLICY_PRODUCTS=3 (bf16 pieces, float32's range) or CAVOID_POLICY_F32=1")
                raise ValueError("%d weight(s) lie beyond +-65504 (after the LSTM gates' log2 e scale): the default float16-split inference "
                                 "form would clamp them.  Create the policy with %s in the environment." % (bad, escape))

    def weights_struct(self, with_backward: bool = False) -> "_lib.CavoidPolicyWeights":
        """``cavoid_policy_weights`` over the module's current parameters (what ``refresh`` loads).  Parameters that are not contiguous
        float32 on the device are handed over as copies, kept alive in ``_keep`` until the next call."""
        n = self.net
        w = _lib.CavoidPolicyWeights()
        w.struct_size = C.sizeof(_lib.CavoidPolicyWeights)
        w.min_policy, w.forget_bias = float(n.min_policy), self.forget_bias
        w.with_backward = 1 if with_backward else 0
        ptr = lambda t: C.c_void_p(self._f32(t).data_ptr())
        self._keep = []                  # tensors that had to be made contiguous stay alive until the next refresh
        if n.normalize:
            w.avg, w.std = ptr(n.avg), ptr(n.std)
        names = ("layer1_kernel", "layer1_bias", "layer2_kernel", "layer2_bias", "fc1_kernel", "fc1_bias", "p_kernel", "p_bias", "v_kernel", "v_bias")
        for name in names if self.ws else ("lstm_kernel", "lstm_bias") + names:      # (weight_sharing: the lstm fields stay NULL)
            setattr(w, name, ptr(getattr(n, name)))
        return w

    def _f32(self, t: torch.Tensor) -> torch.Tensor:
        t = t.detach()
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
            self._keep.append(t)
        return t

    def forward(self, x: torch.Tensor, sample: Optional[bool] = None, greedy: bool = False,
                rows: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, actions_out: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """x float32 [B, input_size] (rows may be strided: a column slice of the env's obs tensor) ->
        (p [B, A], v [B], actions int32 [B] or None).  ``rows`` = (row_index int32 [B], row_count int32 [1]) on the
        device restricts the pass to the listed rows; the others' outputs are zero."""
        if x.dim() != 2 or x.shape[1] != self.input_size or x.dtype != torch.float32 or x.device != self.device:
            raise ValueError("x must be float32 [B, %d] on %s" % (self.input_size, self.device))
        if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < self.input_size):
            x = x.contiguous()
        B = x.shape[0]
        stride = x.stride(0) if B > 1 else self.input_size
        new = torch.zeros if rows is not None else torch.empty
        p = new((B, self.num_actions), dtype=torch.float32, device=self.device)
        v = new((B,), dtype=torch.float32, device=self.device)
        want_actions = greedy if sample is None else (sample or greedy)
        a = new((B,), dtype=torch.int32, device=self.device) if want_actions else None
        if actions_out is not None:                        # with a row list: ONLY the listed rows' actions are overwritten
            if actions_out.dtype != torch.int32 or actions_out.numel() != B or not actions_out.is_contiguous():
                raise ValueError("actions_out must be a contiguous int32 tensor of B elements")
            a = actions_out
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        if rows is None:
            _lib.check(self._lib.cavoid_policy_forward(self._h, ptr(x), B, stride, ptr(p), ptr(v), ptr(a), 1 if greedy else 0,
                                                       self._stream()), "cavoid_policy_forward")
        else:
            _lib.check(self._lib.cavoid_policy_forward_rows(self._h, ptr(x), B, stride, ptr(rows[0]), ptr(rows[1]), ptr(p), ptr(v),
                                                            ptr(a), 1 if greedy else 0, self._stream()), "cavoid_policy_forward_rows")
        return p, v, a

    def __call__(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        p, v, _ = self.forward(x, sample=False)
        return p, v

    def act(self, x: torch.Tensor, greedy: bool = False, rows=None, actions_out=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """predict + select_action (ProcessAgent.py:89-103,128-144): (actions int32 [B], p, v)."""
        p, v, a = self.forward(x, sample=True, greedy=greedy, rows=rows, actions_out=actions_out)
        return a, p, v


# the reference's optimiser options (NetworkVPCore.py:104-122): RMSPROP_DECAY / RMSPROP_MOMENTUM / RMSPROP_EPSILON of Config.py, GRAD_CLIP_NORM
RMSPROP_DEFAULTS = {"decay": 0.99, "momentum": 0.0, "eps": 0.1}
GRAD_CLIP_NORM = 40.0
# the row slices of cavoid_policy_weight_grads (kStepDenseSlice, kStepLstmSlice, kStepLstmSliceWide, kStepLstmWideFrom of
# cavoid_policy_step.hpp -- tests/test_policy_step_host.py holds the scratch size they give to the library's own answer)
STEP_DENSE_SLICE, STEP_LSTM_SLICE, STEP_LSTM_SLICE_WIDE, STEP_LSTM_WIDE_FROM = 1024, 1024, 4096, 4194304


def step_partition(max_others: int, rows: int) -> Tuple[int, int, int]:
    """(dense slices, LSTM slice length, LSTM slices) of ``cavoid_policy_weight_grads`` over ``rows`` buffer rows."""
    t = rows * max_others
    lstm_len = STEP_LSTM_SLICE_WIDE if t > STEP_LSTM_WIDE_FROM else STEP_LSTM_SLICE
    return -(-rows // STEP_DENSE_SLICE), lstm_len, -(-t // lstm_len)


# the row slices of cavoid_policy_weight_grads_ws (kStepWsL1Slice, kStepWsFilterSlice, kStepWsFilterSliceWide, kStepWsFilterWideFrom of
# cavoid_policy_step_ws.hpp -- tests/test_policy_step_ws_host.py holds them to the header's text, tests/test_gpu_policy_step_ws.py the
# scratch size they give to the library's own answer)
STEP_WS_L1_SLICE, STEP_WS_FILTER_SLICE, STEP_WS_FILTER_SLICE_WIDE, STEP_WS_FILTER_WIDE_FROM = 1024, 1024, 4096, 4194304


def step_partition_ws(max_others: int, rows: int) -> Tuple[int, int, int, int, int]:
    """(dense slices, layer1 slice length, layer1 slices, filter slice length, filter slices) of ``cavoid_policy_weight_grads_ws`` over
    ``rows`` buffer rows: the dense slices are STEP_DENSE_SLICE rows, the filter's run over the flat ``max_others * rows`` rows."""
    t = rows * max_others
    l1_len = STEP_WS_L1_SLICE
    f_len = STEP_WS_FILTER_SLICE_WIDE if t > STEP_WS_FILTER_WIDE_FROM else STEP_WS_FILTER_SLICE
    return -(-rows // STEP_DENSE_SLICE), l1_len, -(-rows // l1_len), f_len, -(-t // f_len)


def step_scratch_floats_ws(max_others: int, rows: int) -> int:
    """the floats ``cavoid_policy_weight_grads_scratch_ws`` reports: one partial per slice (include/cavoid.h)"""
    dense, _, l1, _, f = step_partition_ws(max_others, rows)
    return l1 * (4 + 64 * max_others) * 256 + dense * (2 * 65536 + 256 * 16) + f * 8 * 64


class DeviceStepOptimizer(object):
    """What ``FusedA3CTrainer(device_step=True).opt`` (or ``ws_device_step=True``) is: the optimiser whose step is ``cavoid_policy_apply`` (``_ws``)
    -- flat float32 state vectors in the layout of ``cavoid_policy_param_layout`` (``_ws``), a device step count -- behind the part of ``torch.optim.Optimizer``'s surface the training
    loop and the checkpoints use: ``param_groups`` (``lr`` is read from group 0 at every step), ``step``, ``zero_grad``, ``state_dict`` /
    ``load_state_dict``.  'adam': the state dict is ``torch.optim.Adam``'s own, both ways, so a run resumes with or without the device
    step.  'rmsprop': its own format, marked ``"kind": "rmsprop"``."""

    def __init__(self, trainer: "FusedA3CTrainer", kind: str, adam: torch.optim.Adam, learning_rate: float):
        self._trainer, self.kind, self._adam = trainer, kind, adam
        total, dev = trainer._layout[2], trainer.device
        self.state1 = torch.zeros(total, dtype=torch.float32, device=dev)      # Adam: exp_avg; RMSProp: ms
        self.state2 = torch.zeros(total, dtype=torch.float32, device=dev)      # Adam: exp_avg_sq; RMSProp: mom
        self.step_count = torch.zeros(1, dtype=torch.int64, device=dev)
        if kind == "rmsprop":
            for v in trainer._views(self.state1).values():                        # TensorFlow's RMSProp starts ms at ones (the padding stays 0)
                v.fill_(1.0)
            self.param_groups = [dict(RMSPROP_DEFAULTS, lr=float(learning_rate))]
        else:
            self.param_groups = adam.param_groups

    def step(self) -> None:
        self._trainer._apply()

    def zero_grad(self, set_to_none: bool = False) -> None:
        self._trainer._flat_grads.zero_()

    def state_dict(self) -> dict:
        step = int(self.step_count.item())
        if self.kind == "rmsprop":
            return {"kind": "rmsprop", "state": {"ms": self.state1.clone(), "mom": self.state2.clone(), "step": step},
                    "param_groups": [dict(g) for g in self.param_groups]}
        t, adam = self._trainer, self._adam
        adam.state.clear()
        if step > 0:
            m, v = t._views(self.state1), t._views(self.state2)
            for name, prm in t.net.named_parameters():
                adam.state[prm] = {"step": torch.tensor(float(step), dtype=torch.float32, device=t.device),
                                   "exp_avg": m[name].clone(), "exp_avg_sq": v[name].clone()}
        return adam.state_dict()

    def load_state_dict(self, sd: dict) -> None:
        kind = sd.get("kind", "adam")
        if kind != self.kind:
            raise ValueError("the optimizer state is %s's, this trainer steps with %s" % (kind, self.kind))
        t = self._trainer
        if self.kind == "rmsprop":
            self.state1.copy_(sd["state"]["ms"])
            self.state2.copy_(sd["state"]["mom"])
            self.step_count.fill_(int(sd["state"]["step"]))
            for g, saved in zip(self.param_groups, sd["param_groups"]):
                g.update(saved)
            return
        adam = self._adam
        adam.load_state_dict(sd)
        self.param_groups = adam.param_groups
        self.state1.zero_()
        self.state2.zero_()
        m, v, step = t._views(self.state1), t._views(self.state2), 0
        for name, prm in t.net.named_parameters():
            st = adam.state.get(prm)
            if st:
                m[name].copy_(st["exp_avg"])
                v[name].copy_(st["exp_avg_sq"])
                step = int(st["step"])
        self.step_count.fill_(step)


class FusedA3CTrainer(object):
    """``Server.train_model`` (/root/reference/ga3c/GA3C/Server.py:114-124) with the network's forward pass, the A3C loss
    (NetworkVPCore.py:71-100) and the row-local half of the backward pass as two MFMA kernel launches
    (``cavoid_policy_train``); the weight gradients are the library GEMMs ``X^T G`` over all rows (split-K batched), the
    optimiser is the same fused Adam as ``A3CTrainer``.  Gradients equal PyTorch autograd's on ``NetworkVP_rnn.loss`` to
    float32 rounding (tests/test_gpu_policy.py).  ``train_regression`` is the supervised start's step on the same pair with the
    regression loss head (``cavoid_policy_train_regression``; tests/test_gpu_policy_regression.py).
    ``crowd=True`` (opt-in; the step's time against autograd: profiles/policy_crowd_train_timing.txt) accepts an 'rnn' network of MAX_OTHERS + 1 .. MAX_OTHERS_TRAIN observed
    neighbours: the same two calls on a crowd handle, whose forward launch is the ring kernel of cavoid_policy_train_ring.hpp
    (tests/test_gpu_policy_train_ring.py).  Mind ``scratch_bytes``: the pass keeps 3 360 bytes per buffer row and observed neighbour.
    ``ws_crowd=True`` (opt-in; profiles/policy_wsring_timing.txt) does the same for a 'weight_sharing' network of MAX_OTHERS_WS + 1 ..
    MAX_OTHERS_WS_CROWD neighbours: ``cavoid_policy_train_ws`` on a ``FusedPolicy(net, ws_crowd=True)``, whose forward launch is the ring kernel
    of cavoid_policy_wsring.hpp (tests/test_gpu_policy_wsring.py); a ``policy`` that is already such a one has the same effect.  544 bytes per
    buffer row and neighbour.
    ``device_step=True`` (opt-in, 'rnn' only; profiles/policy_device_step_timing.txt) finishes the step inside the library:
    ``cavoid_policy_weight_grads`` forms every gradient in ONE flat tensor in the checkpoint's layout (every parameter's ``.grad`` is a view of
    it, the multi-GPU all-reduce runs on it as it is) and ``cavoid_policy_apply`` takes the optimiser step on the module's own parameter storage
    and re-packs the weights -- no GEMM library, no ``index_select``, no ``torch.optim`` launch behind the two trainer kernels.  With it,
    ``optimizer="rmsprop"`` (the reference's ``tf.train.RMSPropOptimizer``: RMSPROP_DEFAULTS) and ``grad_clip=c`` (``tf.clip_by_average_norm``
    per variable; the reference's GRAD_CLIP_NORM is 40) are available; ``opt`` is then a ``DeviceStepOptimizer``
    (tests/test_gpu_policy_step.py).
    ``ws_device_step=True`` (opt-in, 'weight_sharing' only, with or without ``ws_crowd``; profiles/policy_ws_device_step_timing.txt) is the
    same for the weight-sharing network: ``cavoid_policy_weight_grads_ws`` and ``cavoid_policy_apply_ws`` on the layout of
    ``cavoid_policy_param_layout_ws``; it sets ``device_step``, and everything above holds (tests/test_gpu_policy_step_ws.py)."""

    def __init__(self, net: NetworkVP_rnn, policy: Optional[FusedPolicy] = None, learning_rate: float = 2e-5, group=None,
                 distributed: Optional[bool] = None, crowd: bool = False, ws_crowd: bool = False, device_step: bool = False,
                 optimizer: str = "adam", grad_clip: Optional[float] = None, ws_device_step: bool = False):
        from .network import A3CTrainer
        if optimizer not in ("adam", "rmsprop"):
            raise ValueError("optimizer must be 'adam' or 'rmsprop', not %r" % (optimizer,))
        if grad_clip is not None and not float(grad_clip) > 0.0:
            raise ValueError("grad_clip must be a positive average norm (or None), not %r" % (grad_clip,))
        if not device_step and not ws_device_step and (optimizer != "adam" or grad_clip is not None):
            raise ValueError("optimizer=%r / grad_clip=%r are steps of cavoid_policy_apply: they need device_step=True (the weight_sharing "
                             "network: ws_device_step=True)" % (optimizer, grad_clip))
        if device_step and net.arch == "weight_sharing":
            raise ValueError("device_step=True carries the 'rnn' network only (cavoid_policy_weight_grads is CAVOID_EUNSUPPORTED on a "
                             "weight-sharing handle): the weight_sharing network finishes its step in the library with ws_device_step=True")
        if ws_device_step and net.arch != "weight_sharing":
            raise ValueError("ws_device_step=True carries the 'weight_sharing' network only, not %r: device_step=True is the 'rnn' network's"
                             % (net.arch,))
        self.device_step = bool(device_step) or bool(ws_device_step)
        self.optimizer, self.grad_clip = optimizer, (float(grad_clip) if grad_clip is not None else None)
        self.ws = net.arch == "weight_sharing"          # cavoid_policy_train_ws (limit: FusedPolicy's MAX_OTHERS_WS, or _WS_CROWD)
        self.crowd = bool(crowd) and not self.ws and net.max_others > MAX_OTHERS
        # a weight-sharing network above MAX_OTHERS_WS: when asked to, or when the policy handed over already runs the ring kernels
        self.ws_crowd = (self.ws and MAX_OTHERS_WS < net.max_others <= MAX_OTHERS_WS_CROWD and
                         (bool(ws_crowd) or (policy is not None and policy.ws and policy.crowd)))
        if self.ws and net.max_others > MAX_OTHERS_WS and not self.ws_crowd:
            raise ValueError("the fused trainer carries the weight_sharing network up to %d observed neighbours (kWsMaxOthers), and up to %d "
                             "with ws_crowd=True; the network observes %d: train with A3CTrainer (autograd)"
                             % (MAX_OTHERS_WS, MAX_OTHERS_WS_CROWD, net.max_others))
        if self.crowd and net.max_others > MAX_OTHERS_TRAIN:
            raise ValueError("the fused ring trainer carries up to %d observed neighbours (kPolMaxOthersTrain), the network observes %d: "
                             "train with A3CTrainer (autograd)" % (MAX_OTHERS_TRAIN, net.max_others))
        if not self.ws and not self.crowd and net.max_others > MAX_OTHERS:
            raise ValueError("the fused trainer carries up to %d observed neighbours (kPolMaxOthers), the network observes %d: "
                             "train with A3CTrainer (autograd)" % (MAX_OTHERS, net.max_others))
        self.net = net
        self.policy = policy if policy is not None else FusedPolicy(net, ws_crowd=self.ws_crowd)
        self._base = A3CTrainer(net, learning_rate=learning_rate, group=group, distributed=distributed)
        self.opt = self._base.opt
        self.device = self.policy.device
        self._buffers = {}
        H, A = net.HIDDEN, net.num_actions
        if self.ws:
            self.policy.refresh(with_backward=True)
            if self.device_step:
                self._begin_device_step(_lib.POLICY_PARAM_NAMES_WS, _lib.policy_param_layout_ws(net.max_others, A), optimizer, learning_rate)
            return
        # packed gate column k = 64w + 16 gate + u  <->  checkpoint column c = 64 gate + 16w + u
        c = torch.arange(4 * H, device=self.device)
        gate, w, u = c // H, (c % H) // 16, c % 16
        self._k_of_c = 64 * w + 16 * gate + u
        # packed LSTM gradient [72 rows: 64 hidden, 7 inputs, pad] x [256 packed columns] -> checkpoint layout [7 + 64, 256]
        rows = torch.cat([torch.arange(H, H + net.OTHER), torch.arange(0, H)]).to(self.device)
        self._lstm_flat = (rows.unsqueeze(1) * (4 * H) + self._k_of_c.unsqueeze(0)).reshape(-1)
        self._l1_rows = torch.cat([torch.arange(H, H + net.HOST), torch.arange(0, H)]).to(self.device)
        self.policy.refresh(with_backward=True)
        if self.device_step:
            self._begin_device_step(_lib.POLICY_PARAM_NAMES, _lib.policy_param_layout(net.max_others, A), optimizer, learning_rate)

    def _begin_device_step(self, names, layout, optimizer: str, learning_rate: float) -> None:
        """the flat gradient tensor in `layout` -- (offsets, sizes, total) in the order of `names` --, every ``.grad`` a view of it, and the optimiser"""
        net = self.net
        self._param_names, self._layout = names, layout
        self._flat_grads = torch.zeros(self._layout[2], dtype=torch.float32, device=self.device)
        self._grad_views = self._views(self._flat_grads)
        self._grad_scratch = {}
        for name, prm in net.named_parameters():
            if prm.dtype != torch.float32 or not prm.is_contiguous() or prm.device != self.device:
                raise ValueError("device_step=True updates the module's own storage: %s must be contiguous float32 on %s" % (name, self.device))
            prm.grad = self._grad_views[name]
        self.opt = DeviceStepOptimizer(self, optimizer, self._base.opt, learning_rate)

    def _views(self, flat: torch.Tensor) -> dict:
        """{parameter name: view of ``flat`` in the parameter's shape} by the layout of ``cavoid_policy_param_layout`` (``_ws``)"""
        off, size, _ = self._layout
        return {name: flat[o:o + n].view_as(getattr(self.net, name)) for name, o, n in zip(self._param_names, off, size)}

    def _weight_grads(self, t: dict, cbuf, rows64: int) -> None:
        """``cavoid_policy_weight_grads`` (``_ws``) on the buffers the launch pair just filled: every ``.grad`` (a view of the flat tensor) is set."""
        pol, ws = self.policy, "_ws" if self.ws else ""
        gs = self._grad_scratch.get(rows64)
        if gs is None:
            floats = C.c_int64()
            _lib.check(getattr(pol._lib, "cavoid_policy_weight_grads_scratch" + ws)(pol._h, rows64, C.byref(floats)), "cavoid_policy_weight_grads_scratch" + ws)
            gs = self._grad_scratch[rows64] = torch.empty(int(floats.value), dtype=torch.float32, device=self.device)
            if len(self._grad_scratch) > (2 if self.ws_crowd else 4):
                self._grad_scratch.pop(next(iter(self._grad_scratch)))
        _lib.check(getattr(pol._lib, "cavoid_policy_weight_grads" + ws)(pol._h, C.byref(cbuf), C.c_void_p(gs.data_ptr()), gs.numel(),
                                                                        C.c_void_p(self._flat_grads.data_ptr()), pol._stream()), "cavoid_policy_weight_grads" + ws)
        for name, prm in self.net.named_parameters():      # (a caller's optimiser may have dropped them: zero_grad(set_to_none=True))
            prm.grad = self._grad_views[name]

    def _apply(self) -> None:
        """``cavoid_policy_apply`` (``_ws``): the optimiser step on the module's parameter storage from the flat gradients, then the re-pack."""
        pol, opt = self.policy, self.opt
        g = opt.param_groups[0]
        o = _lib.CavoidPolicyOptimizer()
        o.struct_size = C.sizeof(o)
        if opt.kind == "rmsprop":
            o.kind, o.decay1, o.decay2, o.eps = _lib.OPT_RMSPROP, float(g["decay"]), float(g["momentum"]), float(g["eps"])
        else:
            o.kind, o.decay1, o.decay2, o.eps = _lib.OPT_ADAM, float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])
        o.lr = float(g["lr"])
        o.clip_average_norm = self.grad_clip if self.grad_clip is not None else 0.0
        o.state1, o.state2, o.step = C.c_void_p(opt.state1.data_ptr()), C.c_void_p(opt.state2.data_ptr()), C.c_void_p(opt.step_count.data_ptr())
        w = pol.weights_struct(with_backward=True)
        if pol._keep:
            raise ValueError("device_step=True updates the module's own storage: its parameters must stay contiguous float32 on %s" % (self.device,))
        if self.ws:                                        # (the filter's two variables are not in the struct: the same check for them)
            n = self.net
            if any(t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device for t in (n.other_kernel, n.other_bias)):
                raise ValueError("device_step=True updates the module's own storage: its parameters must stay contiguous float32 on %s" % (self.device,))
            _lib.check(pol._lib.cavoid_policy_apply_ws(pol._h, C.byref(w), C.c_void_p(n.other_kernel.data_ptr()), C.c_void_p(n.other_bias.data_ptr()),
                                                       C.byref(o), C.c_void_p(self._flat_grads.data_ptr()), pol._stream()), "cavoid_policy_apply_ws")
            return
        _lib.check(pol._lib.cavoid_policy_apply(pol._h, C.byref(w), C.byref(o), C.c_void_p(self._flat_grads.data_ptr()), pol._stream()),
                   "cavoid_policy_apply")

    training_step = property(lambda self: self._base.training_step,
                             lambda self, v: setattr(self._base, "training_step", v))
    frame_counter = property(lambda self: self._base.frame_counter)

    @staticmethod
    def buffer_rows(n: int) -> int:
        """Buffer rows of a pass over n rows: a multiple of 2048 (the split-K slice of the weight-gradient GEMMs) once the batch is that
        large, else of the kernels' 64-row tile."""
        return (n + 2047) // 2048 * 2048 if n >= 2048 else (n + 63) // 64 * 64

    @staticmethod
    def scratch_bytes(max_others: int, rows: int, arch: str = "rnn") -> int:
        """Bytes of device memory ``_scratch`` holds for ``rows`` buffer rows (see ``buffer_rows``), without the 4 168 bytes of loss and
        bias gradients.  'rnn': 6 496 + 3 360 M per row -- z1..z3, g1..g3 (6 x 1 024), gh (64), l1_in (288); per observed neighbour h_in (288),
        save (2 048), gl (1 024): 218 KB per row at M = 63.  'weight_sharing': 6 224 + 544 M."""
        if arch == "weight_sharing":
            return rows * (6 * 1024 + 64 + 4 * 4 + (4 * 64 + 32 + 256) * max_others)
        return rows * (6496 + 3360 * max_others)

    def _scratch(self, rows64: int):
        """The pass's buffers for rows64 buffer rows: (tensors by name, the C struct that points at them)."""
        b = self._buffers.get(rows64)
        if b is None:
            M, R = self.net.max_others, rows64
            shapes = {"z1": (R, 256), "z2": (R, 256), "z3": (R, 256), "gh": (R, 16), "loss": (2,), "g1": (R, 256), "g2": (R, 256),
                      "g3": (R, 256), "db": (1040,)}
            if self.ws:
                shapes.update(l1_in=(R, 4 + 64 * M), f_in=(M, R, 8), gf=(M, R, 64))
            else:
                shapes.update(l1_in=(R, 72), h_in=(M, R, 72), save=(R // 64, M, 16, 256, 8), gl=(M, R, 256))
            t = {k: torch.empty(shape, dtype=torch.float32, device=self.device) for k, shape in shapes.items()}
            c = (_lib.CavoidPolicyTrainWsBuffers if self.ws else _lib.CavoidPolicyTrainBuffers)()
            c.struct_size, c.capacity_rows = C.sizeof(c), rows64
            for k, v in t.items():
                setattr(c, k, C.c_void_p(v.data_ptr()))
            b = self._buffers[rows64] = (t, c)
            if len(self._buffers) > (2 if self.crowd or self.ws_crowd else 4):  # keep the cache small: minibatch size + a remainder or two (crowd rows: GBs each)
                self._buffers.pop(next(iter(self._buffers)))
        return b

    @staticmethod
    def _xtg(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
        """x^T g over all rows, split-K (see network._SplitKLinear)."""
        R = x.shape[0]
        S = split_k_factor(R)
        if S == 1:
            return x.t() @ g
        return torch.bmm(x.view(S, R // S, -1).transpose(1, 2), g.view(S, R // S, -1)).sum(dim=0)

    def _pass(self, x: torch.Tensor, y_r: torch.Tensor, a_idx: torch.Tensor, n: int, regression: bool = False):
        """The launch pair on n > 0 rows -- forward + loss head (A3C, or ``regression``: cost_regression) + the row-local backward --
        then the weight-gradient GEMMs it leaves the operands of: every parameter's ``.grad`` is set.  Returns the scratch tensors
        (``loss`` = [cost_p, cost_v], sums over the rows).  x: float32 rows of stride >= input_size."""
        net, pol = self.net, self.policy
        # buffer rows: a multiple of 2048 (the split-K slice of the weight-gradient GEMMs) once the batch is that large;
        # the kernels write every buffer row, rows past n with zero gradients
        rows64 = self.buffer_rows(n)
        t, cbuf = self._scratch(rows64)
        ptr = lambda v: C.c_void_p(v.data_ptr())
        name = "cavoid_policy_train" + ("_regression" if regression else "") + ("_ws" if self.ws else "")
        loss_args = () if regression else (float(net.beta), float(net.log_epsilon))
        _lib.check(getattr(pol._lib, name)(pol._h, ptr(x), n, x.stride(0), ptr(y_r), ptr(a_idx), *loss_args,
                                           C.byref(cbuf), pol._stream()), name)
        if self.device_step:
            self._weight_grads(t, cbuf, rows64)
            return t
        A, H, M = net.num_actions, net.HIDDEN, net.max_others
        xtg = self._xtg
        d_head = xtg(t["z3"], t["gh"])
        net.p_kernel.grad, net.v_kernel.grad = d_head[:, :A].contiguous(), d_head[:, A:A + 1].contiguous()
        db = t["db"]                     # packed bias order: lstm 256 (weight_sharing: other_bias 64) | layer1 | layer2 | fc1 | heads 16
        net.p_bias.grad, net.v_bias.grad = db[1024:1024 + A], db[1024 + A:1025 + A]
        net.fc1_kernel.grad, net.fc1_bias.grad = xtg(t["z2"], t["g3"]), db[768:1024]
        net.layer2_kernel.grad, net.layer2_bias.grad = xtg(t["z1"], t["g2"]), db[512:768]
        d_l1 = xtg(t["l1_in"], t["g1"])
        net.layer1_bias.grad = db[256:512]
        if self.ws:
            net.layer1_kernel.grad = d_l1                                    # rows: host 4, then slot-major (the checkpoint's order)
            net.other_kernel.grad = xtg(t["f_in"].view(M * rows64, 8), t["gf"].view(M * rows64, 64))  # one GEMM over every slot's rows
            net.other_bias.grad = db[:64]
        else:
            net.layer1_kernel.grad = d_l1.index_select(0, self._l1_rows)     # rows: 64 hidden, 4 host, 4 padding
            gl = t["gl"].view(M * rows64, 4 * H)
            d_lstm = xtg(t["h_in"].view(M * rows64, 72), gl)                 # rows: 64 hidden, 7 inputs, 1 padding; packed gate columns
            net.lstm_kernel.grad = d_lstm.reshape(-1).index_select(0, self._lstm_flat).view(H + net.OTHER, 4 * H)
            net.lstm_bias.grad = db[:256].index_select(0, self._k_of_c)
        return t

    def train(self, x: torch.Tensor, y_r: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
        """One optimiser step on the batch.  ``a``: action indices [n] or the reference's one-hot float [n, A].
        Returns the loss (cost_p + cost_v) as a 0-d device tensor: nothing here waits for the GPU."""
        net, pol = self.net, self.policy
        n = int(x.shape[0])
        if self.device_step:
            if n == 0:                                     # (the padding step below: zero gradients, the others' all-reduced ones move the weights)
                self._flat_grads.zero_()
                loss = torch.zeros((), dtype=torch.float32, device=self.device)
            else:
                a_idx = (a.argmax(dim=1) if a.dim() == 2 else a).to(torch.int32).contiguous()
                loss = self._pass(x.to(torch.float32).contiguous(), y_r.to(torch.float32).contiguous(), a_idx, n)["loss"].sum()
            if self._base.distributed:
                import torch.distributed as dist
                dist.all_reduce(self._flat_grads, op=dist.ReduceOp.SUM, group=self._base.group)     # the flat tensor itself: no cat, no clone
            self._apply()                                  # optimiser step + re-pack: actors and the next pass see the new weights
            self._base.training_step += 1
            self._base.frame_counter += n
            return loss
        if n == 0:
            # (multi-GPU padding step: this rank has no rows, but the all-reduced gradients of the others still move its
            #  parameters -- the packed MFMA weights must follow, or this replica's actors keep acting on stale weights)
            loss = torch.as_tensor(self._base.train(x, y_r, a if a.dim() == 2 else
                                                    torch.nn.functional.one_hot(a.long(), net.num_actions).float()), device=self.device)
            pol.refresh(with_backward=True)
            return loss
        x = x.to(torch.float32).contiguous()
        y_r = y_r.to(torch.float32).contiguous()
        a_idx = (a.argmax(dim=1) if a.dim() == 2 else a).to(torch.int32).contiguous()
        loss = self._pass(x, y_r, a_idx, n)["loss"].sum()
        if self._base.distributed:
            self._base._allreduce_grads()
        self.opt.step()
        self._base.training_step += 1
        self._base.frame_counter += n
        pol.refresh(with_backward=True)                    # actors and the next training pass see the new weights
        return loss

    def train_regression(self, x: torch.Tensor, y_r: torch.Tensor, a: torch.Tensor, opt=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """One step of the supervised start (``train_regression_op`` on ``cost_regression``, NetworkVPCore.py:90-100,123) on the fused
        kernels: softmax cross-entropy of the logits with the teacher's action ``a`` (indices [n], or one-hot [n, A]) + cost_v
        against ``y_r``.  Steps ``opt`` (default: the trainer's own Adam) and re-packs the weights.  Returns (cost_p, cost_v), sums
        over the rows, as 0-d device tensors: nothing here waits for the GPU.  The regression phase is per rank by design
        (``regression.pretrain``): no all-reduce, and ``training_step`` / ``frame_counter`` count RL steps only."""
        net, pol = self.net, self.policy
        n = int(x.shape[0])
        if n == 0:
            zero = torch.zeros((), dtype=torch.float32, device=self.device)
            return zero, zero.clone()
        if x.dim() != 2 or x.shape[1] != net.input_size or x.device != self.device:
            raise ValueError("x must be [n, %d] on %s" % (net.input_size, self.device))
        x = x.to(torch.float32)
        if x.stride(1) != 1 or x.stride(0) < net.input_size:                   # (a column slice of wider rows goes in as it is)
            x = x.reshape(n, -1).clone()
        y_r = y_r.to(torch.float32).contiguous()
        a_idx = (a.argmax(dim=1) if a.dim() == 2 else a).to(torch.int32).contiguous()
        loss = self._pass(x, y_r, a_idx, n, regression=True)["loss"].clone()       # (the scratch is the next pass's)
        (opt if opt is not None else self.opt).step()
        if opt is not None or not self.device_step:        # (the device step re-packs itself)
            pol.refresh(with_backward=True)
        return loss[0], loss[1]
