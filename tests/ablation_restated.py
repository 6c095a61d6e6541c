"""Plain torch / NumPy restatement of captum 0.7.0's FeatureAblation and Occlusion as the reference's harness calls them
(evaluatePerturbation.py:171-176) and of the harness's post-processing (:92-97, :181), for the ablation tests.

captum is in neither the reference tree nor the test image, so this is written from its published source and every line is part of
an UNPINNED claim: one input tensor (B, C, H, W), baseline a number or one (C, H, W) tensor, one altered image per
`model(...)` call (perturbations_per_eval=1).  Semantics restated:
  s0 = model(x)[0, t], raw output, fp32;
  feature ablation: ids from mask.min() to mask.max() inclusive, ascending (an absent id still costs a forward and adds 0);
      m = (mask == j) broadcast to the input, x_j = x * (1 - m) + baseline * m in float arithmetic, d_j = s0 - model(x_j)[0, t],
      attr += d_j * m in fp32;
  occlusion: per non-batch dimension count = ceil((dim - window) / stride) + 1 shifts, an int stride applies to every dimension;
      window k starts at ((k % c0) * s0, (k // c0 % c1) * s1, ...) -- the FIRST dimension's shift runs fastest --, is clipped to the
      input; attr += d_k * m_k, weights += m_k, ascending k; result attr / weights.
`batching`: None is captum's flow (every forward has batch 1).  An int n is the engine's pass shape: s0 from ONE forward of all B
inputs, the altered images of all inputs as one flat list (image-major) cut into forwards of n rows.  No engine imports here."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def logits_of(out):
    return out if isinstance(out, torch.Tensor) else out.logits


# ------------------------------------------------------------------------------------------------ the altered images
def feature_ids(mask):
    return list(range(int(mask.min()), int(mask.max()) + 1))


def feature_masks(mask, shape):
    """mask (H, W) / (C, H, W) integer tensor -> one float (C, H, W) 0/1 mask per id, ascending"""
    for j in feature_ids(mask):
        yield (mask == j).expand(shape).to(torch.float32)


def window_counts(shape, window, strides):
    strides = (strides,) * len(shape) if isinstance(strides, int) else tuple(strides)
    for d, w, s in zip(shape, window, strides):
        assert 1 <= w <= d and s >= 1 and (s <= w or w == d), (shape, window, strides)
    return tuple(math.ceil((d - w) / s) + 1 for d, w, s in zip(shape, window, strides)), strides


def window_starts(shape, window, strides):
    """start index of window k in every non-batch dimension, k ascending"""
    counts, strides = window_counts(shape, window, strides)
    out = []
    for k in range(int(np.prod(counts))):
        rem, start = k, []
        for c, s in zip(counts, strides):
            start.append((rem % c) * s)
            rem //= c
        out.append(tuple(start))
    return out


def window_masks(shape, window, strides):
    """one float 0/1 mask of `shape` (C, H, W) per window, ascending k, overhang clipped"""
    for start in window_starts(shape, window, strides):
        m = torch.zeros(shape, dtype=torch.float32)
        m[tuple(slice(a, min(a + w, d)) for a, w, d in zip(start, window, shape))] = 1.0
        yield m


def ablated(x, m, baseline):
    """captum's expression; x (C, H, W), m float 0/1, baseline a number or a (C, H, W) tensor"""
    return x * (1 - m) + baseline * m


# ------------------------------------------------------------------------------------------------ scores -> attribution
def accumulate(s0, scores, masks, weighted):
    """captum's loop over recorded scores, from its zero-initialised totals: attr += (s0 - s_k) * m_k in fp32, ascending k
    [, weights += m_k, attr / weights] -> (C, H, W)"""
    masks = list(masks)
    attr = torch.zeros_like(masks[0])
    weights = torch.zeros_like(masks[0])
    s0 = torch.tensor(float(s0), dtype=torch.float32) if not torch.is_tensor(s0) else s0.to(torch.float32)
    for s, m in zip(scores, masks):
        s = torch.tensor(float(s), dtype=torch.float32) if not torch.is_tensor(s) else s.to(torch.float32)
        attr += (s0 - s) * m
        weights += m
    return attr / weights if weighted else attr


# ------------------------------------------------------------------------------------------------ the flows
def _scores(model, x, targets, masks, baseline, batching):
    """-> (s0 (B,), scores (B, n)) fp32 on x's device; masks: list of float (C, H, W) masks on the host"""
    B, dev = x.shape[0], x.device
    t = torch.as_tensor(targets).reshape(-1).expand(B).to(dev)
    masks = [m.to(dev) for m in masks]
    base = baseline.to(dev) if torch.is_tensor(baseline) else baseline
    with torch.no_grad():
        if batching is None:
            s0 = torch.stack([logits_of(model(x[b:b + 1]))[0, t[b]] for b in range(B)])
            sc = torch.stack([torch.stack([logits_of(model(ablated(x[b], m, base)[None]))[0, t[b]] for m in masks]) for b in range(B)])
            return s0.float(), sc.float()
        s0 = logits_of(model(x)).gather(1, t.view(-1, 1)).squeeze(1)
        rows = [(b, m) for b in range(B) for m in masks]
        out = []
        for lo in range(0, len(rows), int(batching)):
            part = rows[lo:lo + int(batching)]
            batch = torch.stack([ablated(x[b], m, base) for b, m in part])
            tt = torch.stack([t[b] for b, _ in part])
            out.append(logits_of(model(batch)).gather(1, tt.view(-1, 1)).squeeze(1))
        return s0.float(), torch.cat(out).view(B, len(masks)).float()


def _attribute(model, x, targets, masks, baseline, batching, weighted):
    masks = list(masks)
    s0, sc = _scores(model, x, targets, masks, baseline, batching)
    s0, sc = s0.cpu(), sc.cpu()
    return torch.stack([accumulate(s0[b], sc[b], masks, weighted) for b in range(x.shape[0])]), s0, sc


def feature_ablation(model, x, targets, mask, baseline=0, batching=None):
    """-> (attr (B, C, H, W) on the host, s0, scores)"""
    return _attribute(model, x, targets, feature_masks(mask.cpu(), tuple(x.shape[1:])), baseline, batching, False)


def occlusion(model, x, targets, window, strides, baseline=0, batching=None):
    return _attribute(model, x, targets, window_masks(tuple(x.shape[1:]), window, strides), baseline, batching, True)


# ------------------------------------------------------------------------------------------------ the harness's post-processing
def nearest_exact_index(n_in, n_out):
    """source index of every output pixel of F.interpolate(mode='nearest-exact') along one axis"""
    return [min(int(math.floor((i + 0.5) * n_in / n_out)), n_in - 1) for i in range(n_out)]


def downsize(attr, g):
    """(..., H, W) -> (..., g, g): torchvision Resize((g, g), NEAREST_EXACT) (:95)"""
    return F.interpolate(attr, size=(g, g), mode="nearest-exact")


def harness_map(attr, g=14):
    """attr (B, C, H, W) -> (B, H, W): |sum_c resize(downsize(attr))| (:92-97, :173, :181); resize = bilinear, align_corners=False
    (antialias is a no-op when up-sampling)"""
    H, W = attr.shape[-2:]
    up = F.interpolate(downsize(attr.float(), g), size=(H, W), mode="bilinear", align_corners=False)
    return np.abs(np.sum(up.numpy(), axis=1))


def patch_mask(img_hw, num_patches=14):
    """the harness's mask (:96-97)"""
    ids = torch.arange(num_patches ** 2).reshape((num_patches, num_patches))
    side = int(img_hw / num_patches)
    return ids.repeat_interleave(side, dim=0).repeat_interleave(side, dim=1)
