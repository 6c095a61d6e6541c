"""Grad-CAM on the HIP kernels, behind captum's `LayerGradCam` call shape.

The reference calls captum 0.7.0 (evaluatePerturbation.py:147-153):
    LayerGradCam(model, model.layer4).attribute(x, target, relu_attributions=True)   # (1,1,7,7)
then torchvision Resize -> x ones(3,H,W) -> |sum over channels| (:153,:181).  The layer forward
and the backward to the layer stay PyTorch-ROCm; the channel-weighted reduction and the
up-sample are xai_gradcam_f32 / xai_bilinear_up_f32.

Three pieces are shared with guided.py, one copy each: `layer_tensor` (the hook that records the calling thread's layer tensor),
`layer_handles` / `sum_handles` (the gradient of a forked block output) and `gradcam_reduce` (K3, or device torch ops beyond it).
`gradcam_saliency(graphs=True)` replays the whole one-image pass from this thread's hipGraph (`CapturedGradCam`, a
streams.CapturedCall like every other driver's: proven on the caller's first real input, refused -> eager, cached in `_PASSES`).
"""
import contextlib
import math
import threading

import torch

from . import kernels as K
from ._lib import XaiHipError
from .ig import _logits_of, class_targets
from .streams import CapturedCall, ThreadGraphs, backward_turn

GRADCAM_COUNTS = {"captures": 0, "captures_refused": 0, "replayed": 0, "eager": 0}
_PASSES = ThreadGraphs(limit=4)
CAM_RTOL = 1e-4       # outside deterministic mode: MIOpen's kernels differ run to run by <= 1e-6 of the map's maximum here


@contextlib.contextmanager
def layer_tensor(layer, layer_input=False):
    """While active, a forward through `layer` ON THE CALLING THREAD leaves the layer's output (`layer_input`: its first input,
    captum's attribute_to_layer_input) in the yielded dict under "act".  Module hooks are shared by every thread that runs the
    model, so the hook keeps only this thread's tensor; it is removed on exit, also on an exception."""
    kept = {}
    me = threading.get_ident()

    def hook(mod, inp, out=None):
        if threading.get_ident() == me:
            kept["act"] = inp[0] if layer_input else out
    handle = (layer.register_forward_pre_hook if layer_input else layer.register_forward_hook)(hook)
    try:
        yield kept
    finally:
        handle.remove()


def layer_handles(act):
    """A classifier prepared with prepare.fuse_bn_relu(fork_residual=True) hands a block output on as two tensors on one storage
    (act and act._xai_alias) -> the tensors whose gradients add up to the gradient of the activation."""
    alias = getattr(act, "_xai_alias", None)
    return [act] if alias is None else [act, alias]


def sum_handles(grads):
    """the gradients of `layer_handles(act)` -> d score / d act (None when the score depends on none of them)"""
    live = [g for g in grads if g is not None]
    return None if not live else live[0] if len(live) == 1 else live[0] + live[1]


def gradcam_reduce(act, grad, relu=True, channel_sum=True):
    """captum's Grad-CAM reduction: the gradient averaged over every axis after the channel axis weighs the activation, the
    weighted channels are summed (`channel_sum`) -> (B, 1, *spatial), optional ReLU.  A layer of rank >= 3 with at most 1024
    positions per channel is one xai_gradcam_f32 launch (a ViT block's (B, tokens, dim): "channels" = tokens); what that kernel
    does not cover (no channel sum, rank-2 layers, larger maps) is the same expression in device torch ops -- never the CPU."""
    act, grad = act.float().contiguous(), grad.float().contiguous()
    spatial = tuple(act.shape[2:])
    n_pos = math.prod(spatial)
    if channel_sum and act.dim() >= 3 and n_pos <= 1024:
        B, Cc = act.shape[0], act.shape[1]
        return K.gradcam(act.reshape(B, Cc, n_pos, 1), grad.reshape(B, Cc, n_pos, 1), relu=relu).reshape((B, 1) + spatial)
    weights = grad.mean(dim=tuple(range(2, grad.dim())), keepdim=True) if grad.dim() > 2 else grad
    scaled = weights * act
    if channel_sum:
        scaled = scaled.sum(dim=1, keepdim=True)
    return torch.relu(scaled) if relu else scaled


class LayerGradCam:
    def __init__(self, forward_func, layer, device_ids=None):
        self.forward_func = forward_func
        self.layer = layer

    def _act_and_grad(self, inputs, target, additional_forward_args=None, layer_input=False):
        extra = () if additional_forward_args is None else \
            (tuple(additional_forward_args) if isinstance(additional_forward_args, (tuple, list)) else (additional_forward_args,))
        with layer_tensor(self.layer, layer_input) as kept, torch.enable_grad():
            if not inputs.requires_grad:        # captum's apply_gradient_requirements: the layer output
                inputs = inputs.detach().requires_grad_(True)   # needs a graph even with frozen weights
            out = _logits_of(self.forward_func(inputs, *extra))
            if target is None:
                score = out.sum()
            elif torch.is_tensor(target) and (target.is_cuda or (target.dim() > 0 and target.numel() == out.shape[0] > 1)):
                # one class per image, or one class in a device tensor: read on the device (out[:, int(t)] would be an .item() sync)
                score = out.gather(1, target.reshape(-1, 1).to(out.device, torch.int64).expand(out.shape[0], 1)).sum()
            else:
                score = out[:, int(target)].sum()
            act = kept.get("act")
            if not torch.is_tensor(act):
                raise XaiHipError("LayerGradCam: the layer's " + ("input" if layer_input else "output") + " is not a single tensor")
            handles = layer_handles(act)
            with backward_turn(act.device):                   # streams.py: backward passes on autograd's shared device thread take turns
                grad = sum_handles(torch.autograd.grad(score, handles, allow_unused=len(handles) > 1))
            if grad is None:
                raise XaiHipError("LayerGradCam: the score does not depend on the layer")
        return act.detach(), grad.detach()

    def attribute(self, inputs, target=None, additional_forward_args=None, attribute_to_layer_input=False,
                  relu_attributions=False, attr_dim_summation=True):
        """captum 0.7.0's LayerGradCam.attribute for one input tensor and one layer tensor (`gradcam_reduce` of the layer and the
        gradient of the target score with respect to it); with `attr_dim_summation` -> (B,1,*spatial).  The harness's call shape --
        a (B,C,h,w) layer output, summed -- is one xai_gradcam_f32 launch."""
        if not inputs.is_cuda:
            raise XaiHipError("LayerGradCam.attribute needs its input on a HIP device ('cuda:N')")
        act, grad = self._act_and_grad(inputs, target, additional_forward_args, attribute_to_layer_input)
        return gradcam_reduce(act, grad, relu=relu_attributions, channel_sum=attr_dim_summation)


def patch_captum():
    """Opt-in ("captum itself is not replaced or monkey-patched unless asked"): make
    `from captum.attr import LayerGradCam` -- evaluatePerturbation.py:43, the one harness import of the Grad-CAM path that does
    not go through `util.*` -- resolve to the HIP engine's class.  Only that one name of an installed captum is rebound; every
    other captum class stays captum's.  Returns the class that was replaced (None if captum is not importable: nothing to do).
    Asked for either by calling this function before the harness's imports, or by XAI_PATCH_CAPTUM=1 in the environment
    (honoured when the `util` mirror is imported, i.e. at the harness's first `util` import, :17)."""
    try:
        import captum.attr as cattr
    except ImportError:
        return None
    old = getattr(cattr, "LayerGradCam", None)
    if old is LayerGradCam:
        return old
    cattr.LayerGradCam = LayerGradCam
    try:                                            # captum re-exports the class from its defining module as well
        import importlib
        mod = importlib.import_module("captum.attr._core.layer.grad_cam")
        mod.LayerGradCam = LayerGradCam
    except ImportError:
        pass
    return old


def gradcam_saliency(model, layer, inputs, target, out_hw, channels=3, graphs=False):
    """The (B,H,W) map get_CNN_attr produces for "gc": |sum of `channels` copies of the
    up-sampled, ReLU'd cam| (reference evaluatePerturbation.py:147-153,181), fused into the
    up-sample kernel as scale = channels, take_abs.  A layer of higher resolution than `out_hw` along either axis is resized as
    the reference does it, antialiased (`K.resize_bilinear`): K3's plain bilinear is that resize only while no axis shrinks.
    `graphs`: as ONE replay of this thread's hipGraph of the pass (`CapturedGradCam`, kept per model, input shape, layer and
    output size)."""
    if graphs:
        hw = (int(out_hw[0]), int(out_hw[1]))
        cap = _PASSES.get(model, inputs.device, (tuple(inputs.shape), id(layer), hw, channels),
                          lambda: CapturedGradCam(model, layer, inputs, hw, channels))
        return cap(inputs, target)
    cam = LayerGradCam(model, layer).attribute(inputs, target, relu_attributions=True)
    return K.resize_bilinear(cam[:, 0].contiguous(), out_hw[0], out_hw[1], scale=float(channels), take_abs=True)


class CapturedGradCam(CapturedCall):
    """`gradcam_saliency` for a fixed input shape as ONE hipGraph replay.

    A one-image Grad-CAM is launch-bound: ~500 small classifier kernels (forward, backward to the layer) plus K3 take
    ~3 ms of host launches for well under 1 ms of GPU work.  The whole sequence -- classifier forward, autograd to the
    layer, xai_gradcam_f32, xai_bilinear_up_f32 -- runs on static input / target buffers and is replayed per image from a
    hipGraph of exactly that (3.2 ms -> 1.0 ms per image on ResNet-50) once the graph has proven itself on the caller's first
    real input (streams.CapturedCall; a refused graph leaves the eager pass).  `example_input` gives shape and device only.

        cam = CapturedGradCam(model, model.layer4, example_input, (224, 224))
        sal = cam(x, target)            # (B,H,W) on the device, same values as gradcam_saliency(model, layer, x, target, ...)
    """

    def __init__(self, model, layer, example_input, out_hw, channels=3):
        if not example_input.is_cuda:
            raise XaiHipError("CapturedGradCam needs its input on a HIP device ('cuda:N')")
        super().__init__(GRADCAM_COUNTS, (CAM_RTOL,))
        self.model, self.layer, self.out_hw, self.channels = model, layer, (int(out_hw[0]), int(out_hw[1])), channels
        self.x = torch.zeros(tuple(example_input.shape), dtype=torch.float32, device=example_input.device)
        self.tgt = torch.zeros((self.x.shape[0], 1), dtype=torch.int64, device=self.x.device)

    def step(self):
        return (gradcam_saliency(self.model, self.layer, self.x, self.tgt, self.out_hw, self.channels),)

    def _replay(self):
        # The graph holds backward kernels, so a replay from a thread that is not a stream worker takes the device's turn.  The turn
        # wraps the replay ONLY, never run() as a whole: run() captures on its first call, and a capture takes CAPTURE_LOCK and
        # then, inside step(), the turn -- a turn held around run() would take the two locks in the opposite order and can
        # deadlock two caller threads.
        with backward_turn(self.x.device):
            return super()._replay()

    def __call__(self, inputs, target, graphs=True):
        if tuple(inputs.shape) != tuple(self.x.shape):
            raise ValueError(f"captured for inputs of shape {tuple(self.x.shape)}, got {tuple(inputs.shape)}")
        self.x.copy_(inputs.detach(), non_blocking=True)
        self.tgt.copy_(class_targets(target, self.x.shape[0], self.x.device, "CapturedGradCam").view(-1, 1), non_blocking=True)
        (sal,) = self.run() if graphs else self.eager()
        return sal.clone()                                # a replay overwrites the graph's own output
