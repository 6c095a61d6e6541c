"""Adversarial Gradient Integration (reference util/attribution_methods/AGI.py:29-115 and its harness row,
evaluatePerturbation.py:119-139) on the HIP kernels K23-K25.

A pair is one (image, false class) attack.  Pairs are independent, so one classifier pass carries every pair of its images.
Each of the `max_iter` iterations is one step: the reference's Normalize in front of the classifier (torch ops, so autograd returns
gradients with respect to x_cur), a forward, a softmax, two input gradients (of the false class's and of init_pred's probability)
and one K24 launch, which stops pairs whose argmax reached their class and takes the fgsm step of the others.  The iteration count
lives in per-pair state words, so one hipGraph of the step serves every iteration and is replayed `max_iter` times; stopped pairs
still ride along in the pass (their work is wasted, not wrong).  In front of the replays: the initial forward and K23.  Behind
them: K25 sums the pairs' c_delta in class order into step_grad and makes the harness's percentile-clipped map.  The state words
are read once per call, after a synchronize of the calling stream.

`agi_batch` is the multi-image fast path; `test`, `pgd_step`, `fgsm_step`, `pre_processing` and `Normalize` keep the reference's
signatures.
"""
import numpy as np
import torch
import torch.nn as nn

from . import kernels as K
from ._lib import XaiHipError
from .ig import _logits_of, hip_device
from .streams import GRAD_RTOL, CapturedCall, ThreadGraphs, backward_turn, cat_parts, read_back, run_passes

PERCENTILE, UPPERBOUND = 80, 99                   # the harness's percentiles (evaluatePerturbation.py:130-131)
# how the passes ran (diagnostics); pair_iterations: pair-iterations the replays computed, pair_iterations_used: those a pair needed
# (its updates, plus the forward that found its class)
AGI_COUNTS = {"captures": 0, "captures_refused": 0, "replayed": 0, "eager": 0, "pair_iterations": 0, "pair_iterations_used": 0}
_PASSES = ThreadGraphs(limit=4)


class Normalize(nn.Module):
    """(input - mean) / std per channel, with float32 buffers (AGI.py:16-26)."""

    def __init__(self, mean, std):
        super().__init__()
        self.register_buffer("mean", torch.tensor([float(m) for m in mean], dtype=torch.float32))
        self.register_buffer("std", torch.tensor([float(s) for s in std], dtype=torch.float32))

    def forward(self, input):
        return (input - self.mean.reshape(1, -1, 1, 1)) / self.std.reshape(1, -1, 1, 1)


def pre_processing(obs, torch_device):
    """An (H, W, C) image -> (1, C, H, W) float32 tensor on the HIP device `torch_device`, divided by 255 with NumPy first
    (AGI.py:29-37; the harness's image is already in [0, 1], so the attack runs on [0, 1/255]: DESIGN.md section 2)."""
    dev = hip_device(torch_device)
    scaled = np.asarray(obs) / 255
    return torch.tensor(np.expand_dims(np.transpose(scaled, (2, 0, 1)), 0), dtype=torch.float32, device=dev)


def _sign_step_one(image, epsilon, g_adv, g_lab, c_delta):
    """K24's update for one image and one pair, forced (the decision words say 'update')."""
    dev = image.device
    data = image.detach().to(torch.float32).contiguous().view(1, -1)
    x = torch.empty_like(data)
    logits = torch.zeros((1, 1), dtype=torch.float32, device=dev)            # argmax 0 ...
    classes = torch.full((1,), -1, dtype=torch.int32, device=dev)           # ... is not the class: update
    state = torch.tensor([[1, 0, 0, 0]], dtype=torch.int32).to(dev)
    K.agi_step(logits, g_adv.detach().float().contiguous().view(1, -1), g_lab.detach().float().contiguous().view(1, -1), data, classes,
               epsilon, 2, x, c_delta, state)
    return x.view(image.shape)


def fgsm_step(image, epsilon, data_grad_adv, data_grad_lab):
    """(clamp(image + epsilon * sign(data_grad_adv), 0, 1), -data_grad_lab * (that - image)) (AGI.py:39-49), on K24."""
    if not (torch.is_tensor(image) and image.is_cuda):
        raise XaiHipError("fgsm_step needs its image on a HIP device")
    delta = torch.full((1, image.numel()), -0.0, dtype=torch.float32, device=image.device)     # -0 + d == d for every d
    x = _sign_step_one(image, epsilon, data_grad_adv, data_grad_lab, delta)
    return x, delta.view(image.shape)


class _AgiPass(CapturedCall):
    """Static buffers of k images x K classes; one call is the initial forward, K23 and `max_iter` runs of one step (Normalize,
    forward, softmax, two input gradients, K24), replayed from a hipGraph of that step once it has proven itself on the caller's
    first real batch (streams.CapturedCall), then K25."""

    warmup = 1

    def __init__(self, model, k, classes, img_shape, dev, epsilon, max_iter, normalize):
        super().__init__(AGI_COUNTS, (GRAD_RTOL, 0, 0))
        self.model, self.k, self.n_cls, self.epsilon, self.max_iter = model, k, len(classes), float(epsilon), int(max_iter)
        self.max_class = max(classes)
        P = k * self.n_cls
        self.data = torch.zeros((k,) + img_shape, dtype=torch.float32, device=dev)
        self.x = torch.zeros((P,) + img_shape, dtype=torch.float32, device=dev)
        self.cd = torch.zeros_like(self.x)
        self.state = torch.zeros((P, 4), dtype=torch.int32, device=dev)
        self.init_pred = torch.zeros(k, dtype=torch.int64, device=dev)
        self.classes = torch.tensor(classes, dtype=torch.int32).to(dev)
        self.tgt = torch.tensor(list(classes) * k, dtype=torch.int64).view(P, 1).to(dev)
        self.forced = None                                  # one-hot initial logits (pgd_step's given init_pred)
        if normalize is not None:
            c = img_shape[0]
            self.mean = torch.tensor([float(v) for v in normalize[0]], dtype=torch.float32).reshape(1, c, 1, 1).to(dev)
            self.std = torch.tensor([float(v) for v in normalize[1]], dtype=torch.float32).reshape(1, c, 1, 1).to(dev)
        else:
            self.mean = self.std = None

    def _net(self, x):
        return _logits_of(self.model(x if self.mean is None else (x - self.mean) / self.std))

    def step(self):
        xs = self.x.detach().requires_grad_(True)
        logits = self._net(xs)
        p = torch.softmax(logits, dim=1)
        lab = self.init_pred.view(-1, 1).expand(self.k, self.n_cls).reshape(-1, 1)
        p_adv = p.gather(1, self.tgt).squeeze(1)
        p_lab = p.gather(1, lab).squeeze(1)
        with backward_turn(self.x.device):
            (g_adv,) = torch.autograd.grad(p_adv, xs, grad_outputs=torch.ones_like(p_adv), retain_graph=True)
            (g_lab,) = torch.autograd.grad(p_lab, xs, grad_outputs=torch.ones_like(p_lab))
        K.agi_step(logits.detach().float().contiguous(), g_adv.contiguous(), g_lab.contiguous(), self.data, self.classes, self.epsilon,
                   self.max_iter, self.x, self.cd, self.state)

    def compose(self, run):
        if self.forced is not None:
            logits = self.forced
        else:
            with torch.no_grad():
                logits = self._net(self.data).float().contiguous()
        if self.max_class >= logits.shape[1]:
            raise ValueError(f"AGI: class {self.max_class} is not an output of a classifier with {logits.shape[1]} classes")
        K.agi_init(logits, self.data, self.classes, self.init_pred, self.x, self.cd, self.state)
        for _ in range(self.max_iter):
            run()
        return self.cd, self.state, self.init_pred

    def __call__(self, data, graphs=True):
        self.data.copy_(data)
        cd, state, init_pred = self.run() if graphs else self.eager()
        C, H, W = self.data.shape[1:]
        hm = torch.empty((self.k, H, W), dtype=torch.float32, device=self.data.device)
        step_grad = torch.empty_like(self.data)
        K.agi_heatmap(cd, self.k, PERCENTILE, UPPERBOUND, out=hm, step_grad=step_grad)
        return step_grad, init_pred.clone(), state.clone(), hm, self.x


def _check_args(data, false_classes, max_iter):
    if not torch.is_tensor(data) or not data.is_cuda:
        raise XaiHipError("agi_batch needs its input on a HIP device")
    if data.dim() != 4:
        raise ValueError(f"agi_batch: data must be (B, C, H, W), got {tuple(data.shape)}")
    classes = [int(c) for c in false_classes]
    if not classes:
        raise ValueError("agi_batch: no false classes")
    if min(classes) < 0:
        raise ValueError(f"agi_batch: negative class {min(classes)}")
    if int(max_iter) < 1:
        raise ValueError("agi_batch: max_iter must be >= 1")
    return classes


def _attack(data, model, classes, epsilon, max_iter, normalize, images_per_pass, streams, graphs):
    """-> (step_grad, init_pred, state (B*K, 4) int32 on the host, map)"""
    data = data.detach().float().contiguous()
    B, dev, img_shape = data.shape[0], data.device, tuple(data.shape[1:])
    norm = None if normalize is None else (tuple(float(v) for v in normalize[0]), tuple(float(v) for v in normalize[1]))
    use_graphs = bool(graphs)

    def one_pass(lo, hi):
        key = (hi - lo, img_shape, tuple(classes), float(epsilon), int(max_iter), norm)
        p = _PASSES.get(model, dev, key, lambda: _AgiPass(model, hi - lo, classes, img_shape, dev, epsilon, max_iter, norm), cached=use_graphs)
        return p(data[lo:hi], use_graphs)[:4]

    kind = ("agi_batch", id(model), images_per_pass, img_shape, tuple(classes), float(epsilon), int(max_iter), norm, use_graphs)
    step_grad, init_pred, state, hm = cat_parts(run_passes(dev, B, images_per_pass, one_pass, streams, kind))
    host = read_back(state)
    AGI_COUNTS["pair_iterations"] += host.shape[0] * int(max_iter)
    done, reason = host[:, 1], host[:, 2]
    AGI_COUNTS["pair_iterations_used"] += int((done + (reason == 1).int()).sum())
    return step_grad, init_pred, host, hm


def agi_batch(data, model, false_classes, epsilon=0.05, max_iter=20, normalize=None, images_per_pass=None, streams=1, graphs=True,
              want_map=False):
    """AGI of B independent images against the classes `false_classes` (the reference's selected_ids, in order).
    data: (B, C, H, W) on a HIP device, the reference's `data` (in the harness: the [0, 1] image divided by 255).
    normalize: (mean, std) -- the reference's Normalize in front of `model`.
    -> (step_grad (B, C, H, W), init_pred (B,) int64, iterations (B, K) int32 on the host: the fgsm updates each pair made)
       [+ the (B, H, W) harness map |(clip(mean_c step_grad) - q) / (u - q)| with `want_map`].
    An image whose pairs made no update at all has step_grad 0 (the reference's `test` returns (0, 0, 0) for it).
    `images_per_pass` (default: all B): images per classifier pass, each pass with its own static buffers and hipGraph; `streams` > 1:
    the passes run on that many stream workers (streams.py); passes of one size run the same kernels on the same shapes, so the
    result does not depend on `streams`."""
    classes = _check_args(data, false_classes, max_iter)
    step_grad, init_pred, state, hm = _attack(data, model, classes, epsilon, max_iter, normalize, images_per_pass, streams, graphs)
    iters = state[:, 1].reshape(data.shape[0], len(classes)).clone()
    if want_map:
        return step_grad, init_pred, iters, hm.abs()
    return step_grad, init_pred, iters


def pgd_step(image, epsilon, model, init_pred, targeted, max_iter):
    """(c_delta, perturbed_image) of one attack of `image` (1, C, H, W) toward class `targeted` (AGI.py:52-80), on K23/K24;
    c_delta is the int 0 when the attack made no update, as in the reference."""
    if not (torch.is_tensor(image) and image.is_cuda):
        raise XaiHipError("pgd_step needs its image on a HIP device")
    data = image.detach().float().reshape((1,) + tuple(image.shape[-3:])).contiguous()
    if int(max_iter) < 1:
        return 0, image.clone()
    cls = int(targeted.item()) if torch.is_tensor(targeted) else int(targeted)
    pred = int(torch.as_tensor(init_pred).reshape(-1)[0])
    with torch.no_grad():
        logits = _logits_of(model(data)).float()
    n_out = logits.shape[1]
    if not (0 <= cls < n_out and 0 <= pred < n_out):
        raise ValueError(f"pgd_step: classes {cls}, {pred} are not outputs of a classifier with {n_out} classes")
    if cls == pred:                                         # (test never asks for this: it skips its own class)
        if int(logits.argmax(1)[0]) == cls:
            return 0, image.clone()                         # the first forward already predicts the class: break at once
        raise ValueError("pgd_step: targeted equals init_pred, which the classifier does not predict: not supported")
    p = _AgiPass(model, 1, [cls], tuple(data.shape[1:]), data.device, epsilon, max_iter, None)
    p.forced = torch.nn.functional.one_hot(torch.tensor([pred]), n_out).float().to(data.device).contiguous()   # K23 takes init_pred from it
    step_grad, _, state, _, x = p(data, graphs=False)
    if int(state[0, 1]) == 0:
        return 0, x.view(image.shape)
    return step_grad.view(image.shape), x.view(image.shape)


def test(model, device, data, epsilon, topk, selected_ids, max_iter):
    """(init_pred, image (C, H, W), step_grad (C, H, W)) as NumPy arrays, or (0, 0, 0) when no attack made an update
    (AGI.py:83-115).  data: an (H, W, C) image, divided by 255 here as in the reference."""
    x = pre_processing(data, device)
    classes = [int(c) for c in selected_ids]
    if not classes or int(max_iter) < 1:
        return 0, 0, 0
    step_grad, init_pred, iters = agi_batch(x, model, classes, epsilon=epsilon, max_iter=max_iter)
    if int(iters.max()) == 0:
        return 0, 0, 0
    return int(init_pred[0]), x.squeeze().cpu().numpy(), step_grad.squeeze().cpu().numpy()
