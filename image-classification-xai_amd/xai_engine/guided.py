"""Guided Backprop and Guided Grad-CAM (captum 0.7.0 `GuidedBackprop` / `GuidedGradCam` as the reference's harness calls them,
evaluatePerturbation.py:154-163) on the guided forms of the fused backward kernels and K28.

Guided Backprop is the gradient of the raw target logit with respect to the input in which every ReLU hands back
relu(g_out) * (y > 0) instead of g_out * (y > 0); g_out is the COMPLETE gradient of the ReLU's output (at a residual join the sum
of both branches, behind a max-pool the pool's scattered sum).  Guided Grad-CAM multiplies it with the layer's Grad-CAM
(relu_attributions=True, plain gradient) brought to the input size by F.interpolate(mode="nearest").

One forward and ONE backward serve both: the gradient of the score with respect to layer4's output passes through `fc` and
`avgpool` only -- no ReLU -- so it is the same in guided and in plain mode, and `autograd.grad(score, [x, layer_out])` taken in
guided mode yields the guided input gradient and Grad-CAM's plain layer gradient together (captum runs two forwards and two
backwards).  This holds for any layer behind which the classifier has no ReLU; `GuidedGradCam` is meant for that layer.

A classifier prepared with `prepare.fuse_bn_relu` runs the pass through the guided entries of its two backward kernels
(`prepare.guided_relu`).  Any other classifier takes the compatibility path: for the duration of the call a forward hook on every
`nn.ReLU` module puts the clamp, in device torch ops, on the gradient of that module's output.  The hook acts only on tensors
made by the calling thread's forward, so other threads' passes through the same model are untouched.

The hook that records the layer's output, the sum over a forked output's two gradient handles and the Grad-CAM reduction are
gradcam.py's (`layer_tensor`, `layer_handles` / `sum_handles`, `gradcam_reduce`); the pass itself is this module's.
The whole pass -- forward, backward, the Grad-CAM reduction and K28 -- runs on static buffers and is replayed from a hipGraph
once the graph has proven itself on the caller's first real batch (streams.CapturedCall, per host thread).

Parity with captum itself is UNPINNED: captum is not part of the reference tree; the semantics are restated from its published
source in tests/guided_restated.py (unpinned third-party boundaries).
"""
import contextlib
import threading

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import kernels as K
from . import prepare
from ._lib import XaiHipError
from .gradcam import LayerGradCam, gradcam_reduce, layer_handles, layer_tensor, sum_handles
from .ig import _logits_of, check_input, class_targets
from .streams import GRAD_RTOL, CapturedCall, ThreadGraphs, backward_turn

GUIDED_COUNTS = {"captures": 0, "captures_refused": 0, "replayed": 0, "eager": 0}
_PASSES = ThreadGraphs(limit=4)


def _clamp(g):
    """g <= 0 ? +0 : g -- relu() of a gradient, NaN kept: the expression of the guided kernels"""
    return torch.where(g <= 0, torch.zeros((), dtype=g.dtype, device=g.device), g)


def _unfused_relus(model):
    """the nn.ReLU modules a forward of `model` can call: all of them, minus those owned by a block or a stem that
    prepare.fuse_bn_relu has taken over (their ReLUs run inside the fused kernels, the modules are never called)"""
    if not isinstance(model, nn.Module):
        return []
    fused_forwards = (prepare._fused_block_forward, prepare._fused_resnet_forward)
    skip = set()
    for mod in model.modules():
        if getattr(mod.forward, "__func__", None) in fused_forwards:
            skip.update(id(c) for c in mod.children() if isinstance(c, nn.ReLU))
    return [m for m in model.modules() if isinstance(m, nn.ReLU) and id(m) not in skip]


def _refuse_inplace(model):
    """-> the nn.ReLU modules to hook; XaiHipError when one of them works in place"""
    relus = _unfused_relus(model)
    if any(m.inplace for m in relus):
        raise XaiHipError("guided backprop: the classifier calls nn.ReLU(inplace=True) modules, whose output gradient cannot be "
                          "hooked (captum's GuidedBackprop fails on them too); prepare the classifier with "
                          "xai_engine.prepare.fuse_bn_relu (its fused path never calls the ReLU modules) or use inplace=False")
    return relus


@contextlib.contextmanager
def _guided_modules(model):
    """Compatibility path: while active, the output of every nn.ReLU module called by THIS thread's forward carries a gradient
    hook with the clamp (a tensor hook sees the summed gradient of all consumers of that output, which is what captum's
    backward-pre-hook on the module sees).  Removed on exit, also on an exception."""
    relus = _refuse_inplace(model)
    me = threading.get_ident()

    def hook(mod, inp, out):
        if threading.get_ident() == me and torch.is_tensor(out) and out.requires_grad:
            out.register_hook(_clamp)
    handles = [m.register_forward_hook(hook) for m in relus]
    try:
        yield
    finally:
        for h in handles:
            h.remove()


def guided_gradients(x, model, tgt, layer=None, guided=True):
    """One forward and one backward -> (d score / d x, layer output or None, d score / d layer output or None) with
    score = sum_b logits[b, tgt[b]]; `guided`: every ReLU backpropagates by Guided Backprop's rule.  x (B, ...) and tgt (B, 1)
    int64 on the device.  A layer output forked by fuse_bn_relu(fork_residual=True) gets the sum over its two handles."""
    with contextlib.ExitStack() as stack:
        kept = {} if layer is None else stack.enter_context(layer_tensor(layer))
        stack.enter_context(torch.enable_grad())
        if guided:
            stack.enter_context(prepare.guided_relu())
            stack.enter_context(_guided_modules(model))
        xs = x.detach().requires_grad_(True)
        out = _logits_of(model(xs))
        score = out.gather(1, tgt).sum()
        if layer is None:
            with backward_turn(x.device):
                (gx,) = torch.autograd.grad(score, xs)
            return gx.detach(), None, None
        act = kept.get("act")
        if not torch.is_tensor(act):
            raise XaiHipError("guided Grad-CAM: the layer's output is not a single tensor")
        with backward_turn(x.device):
            grads = torch.autograd.grad(score, [xs] + layer_handles(act), allow_unused=True)
    g_act = sum_handles(grads[1:])
    if grads[0] is None or g_act is None:
        raise XaiHipError("guided Grad-CAM: the score does not depend on the input through the layer")
    return grads[0].detach(), act.detach(), g_act.detach()


class _GuidedPass(CapturedCall):
    """Static input and target buffers of one input shape; a call is forward + guided backward (+ Grad-CAM reduction) + K28,
    replayed from a hipGraph of exactly that once it has proven itself on the caller's first real batch (streams.CapturedCall)."""

    def __init__(self, model, layer, shape, dev, want_attr, want_map):
        super().__init__(GUIDED_COUNTS, (GRAD_RTOL,) * (int(want_attr) + int(want_map)))
        self.model, self.layer, self.want_attr, self.want_map = model, layer, want_attr, want_map
        self.x = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.tgt = torch.zeros((shape[0], 1), dtype=torch.int64, device=dev)

    def step(self):
        gx, act, g_act = guided_gradients(self.x, self.model, self.tgt, self.layer)
        cam = None
        if self.layer is not None:
            if act.dim() != 4:
                raise XaiHipError(f"guided Grad-CAM needs a (B, C, h, w) layer output, got {tuple(act.shape)}")
            cam = gradcam_reduce(act, g_act, relu=True)[:, 0]         # LayerGradCam(..., relu_attributions=True) -> (B, h, w)
        out = K.guided_map(gx.float().contiguous(), cam, want_attr=self.want_attr, want_map=self.want_map)
        return out if isinstance(out, tuple) else (out,)

    def __call__(self, x, tgt, graphs):
        self.x.copy_(x)
        self.tgt.copy_(tgt.view(-1, 1))
        out = self.run() if graphs else self.eager()
        return tuple(t.clone() for t in out)             # a replay overwrites the graph's own outputs


def guided_backprop_batch(x, model, targets, layer=None, want_attr=True, want_map=False, graphs=True):
    """Guided Backprop of B images in one classifier pass: x (B, C, H, W) on a HIP device, `targets` one class index or one per
    image (a device tensor is not read back); score = sum_b logits[b, targets[b]], so every image gets the guided gradient of its
    own logit.  With `layer` (a module with a (B, C, h, w) output, the harness's model.layer4): Guided Grad-CAM, that gradient
    times the nearest-upsampled Grad-CAM of the layer, from the same single backward.
    -> the attribution (B, C, H, W) (`want_attr`), the harness's map |sum over channels| (B, H, W) (`want_map`), or (attr, map).
    `graphs`: replay the pass from a hipGraph, kept per thread, model, input shape and layer."""
    x = check_input(x, "guided_backprop_batch")
    if not (want_attr or want_map):
        raise ValueError("guided_backprop_batch: nothing to return (neither want_attr nor want_map)")
    dev, shape = x.device, tuple(x.shape)
    tgt = class_targets(targets, shape[0], dev, "guided_backprop_batch").view(-1, 1)
    _refuse_inplace(model)                                # before any buffer or graph is made
    key = (shape, None if layer is None else id(layer), bool(want_attr), bool(want_map))
    p = _PASSES.get(model, dev, key, lambda: _GuidedPass(model, layer, shape, dev, bool(want_attr), bool(want_map)), cached=bool(graphs))
    out = p(x, tgt, bool(graphs))
    return out if len(out) > 1 else out[0]


def _forward_args(model, additional_forward_args):
    if additional_forward_args is None:
        return model
    extra = tuple(additional_forward_args) if isinstance(additional_forward_args, (tuple, list)) else (additional_forward_args,)
    return _WithArgs(model, extra)


class _WithArgs(nn.Module):
    """model(x, *extra) as a one-argument module (captum's additional_forward_args); the ReLU modules stay reachable"""

    def __init__(self, model, extra):
        super().__init__()
        self.model, self.extra = model, extra

    def forward(self, x):
        return self.model(x, *self.extra)


class GuidedBackprop:
    """captum.attr.GuidedBackprop's call shape on the HIP path, for what the harness uses (evaluatePerturbation.py:154-158)."""

    def __init__(self, model):
        self.model = model

    def attribute(self, inputs, target=None, additional_forward_args=None):
        """-> (B, C, H, W) device tensor"""
        return guided_backprop_batch(inputs, _forward_args(self.model, additional_forward_args), target,
                                     graphs=additional_forward_args is None)


class GuidedGradCam:
    """captum.attr.GuidedGradCam's call shape on the HIP path, for what the harness uses (evaluatePerturbation.py:159-163)."""

    def __init__(self, model, layer, device_ids=None):
        self.model = model
        self.layer = layer

    def attribute(self, inputs, target=None, additional_forward_args=None, interpolate_mode="nearest", attribute_to_layer_input=False):
        """-> (B, C, H, W) device tensor.  The harness's call (`nearest`, the layer's output) is one captured pass ending in K28;
        another `interpolate_mode` or `attribute_to_layer_input=True` is the same product in device torch ops -- never the CPU."""
        model = _forward_args(self.model, additional_forward_args)
        if interpolate_mode == "nearest" and not attribute_to_layer_input:
            return guided_backprop_batch(inputs, model, target, layer=self.layer, graphs=additional_forward_args is None)
        x = check_input(inputs, "GuidedGradCam.attribute")
        tgt = class_targets(target, x.shape[0], x.device, "GuidedGradCam.attribute")
        gx, _, _ = guided_gradients(x, model, tgt.view(-1, 1))
        cam = LayerGradCam(model, self.layer).attribute(x, tgt, attribute_to_layer_input=attribute_to_layer_input, relu_attributions=True)
        return gx * F.interpolate(cam, x.shape[2:], mode=interpolate_mode)


def patch_captum():
    """Opt-in, like ablation.patch_captum and separate from gradcam.patch_captum (which stays LayerGradCam's alone): make
    `from captum.attr import GuidedBackprop, GuidedGradCam` -- evaluatePerturbation.py:43 -- resolve to the classes above.  Only these
    two names of an installed captum's `captum.attr` are rebound.  -> the (GuidedBackprop, GuidedGradCam) pair that was replaced, or
    None when captum is not importable."""
    try:
        import captum.attr as cattr
    except ImportError:
        return None
    old = (getattr(cattr, "GuidedBackprop", None), getattr(cattr, "GuidedGradCam", None))
    cattr.GuidedBackprop, cattr.GuidedGradCam = GuidedBackprop, GuidedGradCam
    return old
