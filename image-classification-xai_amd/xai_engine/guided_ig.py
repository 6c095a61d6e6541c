"""Guided IG (reference util/attribution_methods/GIGBuilder.py:194-310) on the HIP step kernel K22.

Each of the `steps` outer steps is one classifier forward pass, a softmax, one backward pass (the gradient of the target's
softmax PROBABILITY, not its logit: call_model_function, :296-310), then one launch of xai_gig_step_f32, which runs the step's
whole inner `while gamma > 1` loop on the device.  Nothing comes back to the host between steps: the step index lives in
per-image state words that the kernel advances, so one hipGraph of "pass + K22" serves every step and is replayed `steps` times.
The state words are read once per call, after a synchronize of the calling stream; a nonzero status raises XaiHipError.

`guided_ig_batch` is the multi-image fast path (images are independent: one workgroup of K22 per image, one classifier pass for
all of them); `GuidedIG.GetMask` keeps the reference's signature (the mirror module util/attribution_methods/GIGBuilder.py
serves it).
"""
import torch

from . import kernels as K
from ._lib import XaiHipError
from .ig import _logits_of, abs_channel_sum, hip_device
from .streams import GRAD_RTOL, CapturedCall, ThreadGraphs, backward_turn, cat_parts, read_back, run_passes

INPUT_OUTPUT_GRADIENTS = "INPUT_OUTPUT_GRADIENTS"      # the key of GIGBuilder.py:15
GIG_COUNTS = {"captures": 0, "captures_refused": 0, "replayed": 0, "eager": 0}     # how the passes ran (diagnostics)
_PASSES = ThreadGraphs(limit=4)


def softmax_grad(model, x, targets):
    """d softmax(model(x))[i, targets[i]] / dx for a batch (targets: (B,) long on x's device)."""
    xs = x.detach().requires_grad_(True)
    p = torch.softmax(_logits_of(model(xs)), dim=1).gather(1, targets.view(-1, 1)).squeeze(1)
    with backward_turn(x.device):
        (g,) = torch.autograd.grad(p, xs, grad_outputs=torch.ones_like(p))
    return g.contiguous()


class _GigPass(CapturedCall):
    """Static buffers of k images; one call is K22's init and `steps` runs of one step (forward, softmax, backward, K22), replayed
    from a hipGraph of that step once it has proven itself on the caller's first real batch (streams.CapturedCall)."""

    warmup = 1                                            # the eager call runs the step `steps` times before the capture

    def __init__(self, model, k, img_shape, dev, steps, fraction, max_dist):
        super().__init__(GIG_COUNTS, (GRAD_RTOL, 0))
        self.model, self.steps, self.fraction, self.max_dist = model, steps, fraction, max_dist
        self.xin = torch.zeros((k,) + img_shape, dtype=torch.float32, device=dev)
        self.base = torch.zeros_like(self.xin)
        self.x = torch.zeros_like(self.xin)
        self.attr = torch.zeros_like(self.xin)
        self.l1 = torch.zeros(k, dtype=torch.float32, device=dev)
        self.state = torch.zeros((k, 4), dtype=torch.int32, device=dev)
        self.t = torch.zeros(k, dtype=torch.int64, device=dev)

    def step(self):
        g = softmax_grad(self.model, self.x, self.t)
        K.gig_step(self.xin, self.base, g, self.steps, self.fraction, self.max_dist, self.x, self.attr, self.l1, self.state)

    def compose(self, run):
        K.gig_init(self.xin, self.base, self.x, self.attr, self.l1, self.state)
        for _ in range(self.steps):
            run()
        return self.attr, self.state

    def __call__(self, xin, base, targets, graphs=True):
        self.xin.copy_(xin)
        self.base.copy_(base)
        self.t.copy_(targets)
        attr, state = self.run() if graphs else self.eager()
        return attr.clone(), state.clone()


def _raise_on_status(state, first=0):
    """state: (B, 4) int32 on the host."""
    for i, (step, status, sel, at) in enumerate(state.tolist()):
        if status != 0:
            raise XaiHipError(f"guided IG: image {first + i}: status {status} at step {at} after {sel} selections: "
                              f"{K.GIG_STATUS.get(status, 'unknown status')}")


def _check_args(steps, fraction):
    if int(steps) < 1:
        raise ValueError("steps must be >= 1")
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError("fraction must be in [0, 1]")


def guided_ig_batch(x, model, targets, steps=50, fraction=0.25, max_dist=0.02, baseline=0, want_abs=False, streams=1,
                    images_per_pass=None, graphs=True):
    """Guided IG of B independent images: x (B,C,H,W) on a HIP device, targets (B,) long -> attribution (B,C,H,W)
    [and, with want_abs, the (B,H,W) |sum_c| map the metrics consume].
    `baseline`: a python number or a tensor of x's shape (or broadcastable to it).
    `images_per_pass` (default: all B): images per classifier pass; every pass has its own static buffers and, with `graphs`, its
    own hipGraph of one step, replayed `steps` times.  `streams` > 1: the passes run on that many stream workers (streams.py), each
    replaying a graph it captured itself; passes of the same size run the same kernels on the same shapes, so the result does not
    depend on `streams`."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise XaiHipError("guided_ig_batch needs its input on a HIP device")
    _check_args(steps, fraction)
    x = x.detach().float().contiguous()
    B, dev, img_shape = x.shape[0], x.device, tuple(x.shape[1:])
    if torch.is_tensor(baseline):
        base = baseline.detach().to(dev, torch.float32).expand_as(x).contiguous()
    else:
        base = torch.full_like(x, float(baseline))
    targets = targets.to(dev).long().reshape(B)

    def one_pass(lo, hi):
        key = (hi - lo, img_shape, int(steps), float(fraction), float(max_dist))
        p = _PASSES.get(model, dev, key, lambda: _GigPass(model, hi - lo, img_shape, dev, steps, fraction, max_dist), cached=graphs)
        return p(x[lo:hi], base[lo:hi], targets[lo:hi], graphs)

    kind = ("guided_ig_batch", id(model), images_per_pass, img_shape, int(steps), float(fraction), float(max_dist), bool(graphs))
    attr, state = cat_parts(run_passes(dev, B, images_per_pass, one_pass, streams, kind))
    _raise_on_status(read_back(state))
    if not want_abs:
        return attr
    return attr, (abs_channel_sum(attr) if attr.shape[1] == 3 else attr.sum(1).abs())


def _is_builtin(fn):
    """The reference's call_model_function (GIGBuilder.py:296) or this module's."""
    return fn is call_model_function or (getattr(fn, "__name__", "") == "call_model_function"
                                         and getattr(fn, "__module__", "").split(".")[-1].startswith("GIGBuilder"))


def call_model_function(images, model, device, call_model_args=None, expected_keys=None):
    """The gradient of the target class's softmax probability with respect to `images` (GIGBuilder.py:296-310), computed on
    `device`; returned under INPUT_OUTPUT_GRADIENTS on `device`."""
    dev = hip_device(device)
    x = images.detach().to(dev, torch.float32)
    t = torch.full((x.shape[0],), int(call_model_args["class_idx_str"]), dtype=torch.int64, device=dev)
    if expected_keys is not None and INPUT_OUTPUT_GRADIENTS in expected_keys:
        return {INPUT_OUTPUT_GRADIENTS: softmax_grad(model, x, t)}
    return {}


class GuidedIG:
    """Guided IG with the reference's interface (GIGBuilder.py:312-372), on the HIP device `device`."""

    expected_keys = [INPUT_OUTPUT_GRADIENTS]

    def GetMask(self, x_value, model, device, call_model_function, call_model_args=None,
                x_baseline=None, x_steps=200, fraction=0.25, max_dist=0.02):
        """The Guided IG attribution of x_value (shape and device of x_value); the work runs on `device`.  With the reference's
        (or this module's) call_model_function and a batch of one, the steps are replayed from a hipGraph (guided_ig_batch);
        any other gradient function is called once per step, eagerly, each call followed by K22."""
        dev = hip_device(device)
        _check_args(x_steps, fraction)
        if x_baseline is None:
            x_baseline = torch.zeros_like(x_value)
        if tuple(x_baseline.shape) != tuple(x_value.shape):
            raise ValueError(f"x_baseline has shape {tuple(x_baseline.shape)}, x_value {tuple(x_value.shape)}")
        x = x_value.detach().to(dev, torch.float32).contiguous()
        base = x_baseline.detach().to(dev, torch.float32).contiguous()
        if _is_builtin(call_model_function) and x.dim() >= 2 and x.shape[0] == 1:
            t = torch.tensor([int(call_model_args["class_idx_str"])], dtype=torch.int64).to(dev)
            attr = guided_ig_batch(x, model, t, steps=x_steps, fraction=fraction, max_dist=max_dist, baseline=base)
            return attr.to(x_value.device)
        # the whole of x_value is one point of the path (the reference's l1 distances and quantile span every element)
        n = x.numel()
        xin, b = x.reshape(1, n), base.reshape(1, n)
        xcur, attr = torch.empty_like(xin), torch.empty_like(xin)
        l1 = torch.empty(1, dtype=torch.float32, device=dev)
        state = torch.empty((1, 4), dtype=torch.int32, device=dev)
        K.gig_init(xin, b, xcur, attr, l1, state)
        for _ in range(int(x_steps)):
            if _is_builtin(call_model_function):
                t = torch.full((x.shape[0],), int(call_model_args["class_idx_str"]), dtype=torch.int64, device=dev)
                g = softmax_grad(model, xcur.view(x.shape), t)
            else:
                out = call_model_function(xcur.view(x.shape).clone().to(x_value.device), model, device,
                                          call_model_args=call_model_args, expected_keys=self.expected_keys)
                g = out[INPUT_OUTPUT_GRADIENTS]
            g = g.detach().to(dev, torch.float32).reshape(1, n).contiguous()
            K.gig_step(xin, b, g, x_steps, fraction, max_dist, xcur, attr, l1, state)
        torch.cuda.current_stream(dev).synchronize()
        _raise_on_status(state.cpu())
        return attr.view(x.shape).to(x_value.device)
