"""Guided Backprop and Guided Grad-CAM restated in plain torch (not a test; imports nothing from the engine).

captum is on no machine of this project, so what its 0.7.0 release computes is restated here from its published source; parity
with captum itself stays unpinned.  What is restated, by file and function of captum 0.7.0 (the source is not at
hand, so no line numbers are claimed):

  captum/attr/_core/guided_backprop_deconvnet.py
    ModifiedReluGradientAttribution.attribute   hooks on every torch.nn.ReLU module of the model, then the plain gradient of the
                                                target output with respect to the inputs (summed over the batch: one backward),
                                                hooks removed in a finally
    GuidedBackprop._backward_hook               the gradient handed on by a ReLU is F.relu() of what the plain rule hands on:
                                                relu(g_out * (y > 0)) == relu(g_out) * (y > 0)            -> `guided_backprop`
  captum/attr/_core/guided_grad_cam.py
    GuidedGradCam.attribute                     LayerGradCam(model, layer).attribute(..., relu_attributions=True) of the layer
                                                OUTPUT, from a plain forward and backward of its own; GuidedBackprop of the inputs;
                                                their product after LayerAttribution.interpolate(cam, inputs.shape[2:],
                                                interpolate_mode="nearest") == F.interpolate(..., mode="nearest")
                                                                                                          -> `guided_gradcam`
  captum/attr/_core/layer/grad_cam.py
    LayerGradCam.attribute                      mean of the layer gradient over the spatial axes, times the layer output, summed
                                                over channels (keepdim), relu                             -> `gradcam`

and the reference harness's evaluatePerturbation.py:181, np.abs(np.sum(attr, axis=0))                      -> `harness_map`.
The clamp is written as a backward-pre-hook on the module: it replaces g_out, the complete gradient of the ReLU's output, before
the ReLU's own backward applies the gate.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


def _clamp_grad_output(module, grad_output):
    return tuple(None if g is None else F.relu(g) for g in grad_output)


def _score(model, x, t):
    out = model(x)
    t = torch.as_tensor(t, device=out.device).reshape(-1).expand(out.shape[0])
    return out.gather(1, t.view(-1, 1)).sum()


def guided_backprop(model, x, t):
    """(B, C, H, W): d sum_b model(x)[b, t_b] / d x with relu(g_out) in front of every nn.ReLU module's backward"""
    relus = [m for m in model.modules() if isinstance(m, nn.ReLU)]
    assert relus and not any(m.inplace for m in relus)
    handles = [m.register_full_backward_pre_hook(_clamp_grad_output) for m in relus]
    try:
        with torch.enable_grad():
            xr = x.detach().clone().requires_grad_(True)
            (g,) = torch.autograd.grad(_score(model, xr, t), xr)
    finally:
        for h in handles:
            h.remove()
    return g.detach()


def layer_act_and_grad(model, layer, x, t):
    """(layer output, plain gradient of the score with respect to it)"""
    kept = {}
    handle = layer.register_forward_hook(lambda mod, inp, out: kept.__setitem__("act", out))
    try:
        with torch.enable_grad():
            xr = x.detach().clone().requires_grad_(True)
            score = _score(model, xr, t)
            (g,) = torch.autograd.grad(score, kept["act"])
    finally:
        handle.remove()
    return kept["act"].detach(), g.detach()


def gradcam(model, layer, x, t):
    """(B, 1, h, w): LayerGradCam.attribute(x, t, relu_attributions=True)"""
    act, g = layer_act_and_grad(model, layer, x, t)
    return torch.relu((g.mean(dim=(2, 3), keepdim=True) * act).sum(dim=1, keepdim=True))


def guided_gradcam(model, layer, x, t):
    """(B, C, H, W): two forwards and two backwards, as captum runs them"""
    return guided_backprop(model, x, t) * F.interpolate(gradcam(model, layer, x, t), x.shape[2:], mode="nearest")


def harness_map(attr):
    """(C, H, W) attribution of one image -> the (H, W) map of evaluatePerturbation.py:181"""
    return np.abs(np.sum(attr.detach().cpu().numpy(), axis=0))


def nearest_index(n_in, n_out):
    """source index of every destination index under F.interpolate(mode="nearest") (the legacy rule, not nearest-exact):
    min(int(floor(dst * scale)), n_in - 1) with scale = n_in / n_out and the product both rounded to fp32"""
    scale = np.float32(n_in) / np.float32(n_out)
    return [min(int(np.floor(np.float32(d) * scale)), n_in - 1) for d in range(n_out)]
