"""Feature Ablation and Occlusion (captum 0.7.0 `FeatureAblation` / `Occlusion` as the reference's harness calls them,
evaluatePerturbation.py:171-176) on the HIP kernels K26 / K27.

captum's flow runs one altered image per classifier call (`perturbations_per_eval=1`), builds each with four full-size torch ops
and reads every score back before the next one: 1 + 196 batch-1 forwards for the harness's `fa`, 1 + 36 for `occ`.  Here the altered
images of ALL inputs of a call form one flat list (row = image * n_total + feature or window index); the list is cut into classifier
passes of `pass_size` rows, K26 writes a pass's rows straight into the pass's static input buffer, the forward runs under `no_grad`
(through the fused inference stem when the classifier was prepared with `prepare.fuse_bn_relu`), the target logit of every row is
gathered on the device, and one K27 launch turns the scores into captum's attribution and, for the harness, its 14 x 14 nearest-exact
samples.  Nothing is read back and nothing waits between passes.  Every distinct pass size is one hipGraph (streams.CapturedCall,
per host thread); with `streams` > 1 the passes run on that many stream workers.

`feature_ablation_batch` / `occlusion_batch` are the multi-image entries; `FeatureAblation` / `Occlusion` keep captum's call shape
for what the harness uses (one input tensor, a feature mask shared by the batch, windows spanning all channels);
`patch_captum()` is the opt-in overlay for these two names (gradcam.patch_captum stays the one for LayerGradCam).

Parity with captum itself is UNPINNED: captum is not part of the reference tree; the semantics are restated from its published
source in tests/ablation_restated.py (unpinned third-party boundaries).
"""
import collections
import threading

import torch

from . import kernels as K
from .ig import _logits_of, abs_channel_sum, check_input, class_targets
from .streams import LOGIT_RTOL, CapturedCall, ThreadGraphs, run_passes

PASS_SIZE = 98                     # rows per classifier pass: the harness's 196 patches are two passes, its 36 windows one
NUM_PATCHES = 14                   # the harness's patch grid (evaluatePerturbation.py:94)
OCC_WINDOW, OCC_STRIDE = (3, 64, 64), 32          # the harness's occlusion arguments (:176)
ABLATION_COUNTS = {"captures": 0, "captures_refused": 0, "replayed": 0, "eager": 0, "rows": 0}
_PASSES = ThreadGraphs(limit=4)

PreparedMask = collections.namedtuple("PreparedMask", "ids id_min n_total")    # ids: int32 (H, W) or (C, H, W) on the device


class _ScorePass(CapturedCall):
    """The forward of `b` rows on a static input buffer `x` (K26 writes the rows into it) and the gather of each row's target logit
    from the static `tgt`, replayed as one hipGraph by the thread that captured it once the replay has proven itself on the
    caller's first real rows (streams.CapturedCall)."""

    def __init__(self, model, b, img_shape, dev):
        super().__init__(ABLATION_COUNTS, (LOGIT_RTOL,))
        self.model = model
        self.x = torch.zeros((b,) + tuple(img_shape), dtype=torch.float32, device=dev)
        self.tgt = torch.zeros((b, 1), dtype=torch.int64, device=dev)

    def step(self):
        with torch.no_grad():
            return (_logits_of(self.model(self.x)).float().gather(1, self.tgt).squeeze(1),)


def _baseline(baselines, x, name):
    """None / number / (C, H, W) / (1, C, H, W) -> number or float32 (C, H, W) device tensor"""
    if baselines is None:
        return 0.0
    if isinstance(baselines, (tuple, list)):
        raise NotImplementedError(f"{name}: a tuple of baselines is not supported")
    if not torch.is_tensor(baselines):
        return float(baselines)
    if baselines.numel() == 1 and not baselines.is_cuda:
        return float(baselines)
    b = baselines
    if b.dim() == 4 and b.shape[0] == 1:
        b = b[0]
    if tuple(b.shape) != tuple(x.shape[1:]):
        raise NotImplementedError(f"{name}: a baseline must be a number or one {tuple(x.shape[1:])} tensor shared by the batch, "
                                  f"got {tuple(baselines.shape)}")
    return b.to(x.device, torch.float32).contiguous()


def prepare_mask(feature_mask, shape, dev):
    """captum's feature_mask for inputs of `shape` (B, C, H, W) -> PreparedMask: the int32 id plane on the device and the id range
    [min, max] captum walks.  Accepted: (H, W), (1, H, W), (C, H, W), (1, 1, H, W), (1, C, H, W); None = every element its own
    feature (captum's default).  The range of a HOST mask is taken on the host; a device mask costs one read-back here, before any
    pass.  A PreparedMask is passed through: callers that reuse a mask (the harness) prepare it once."""
    if isinstance(feature_mask, PreparedMask):
        return feature_mask
    B, C, H, W = (int(v) for v in shape)
    if feature_mask is None:
        return PreparedMask(torch.arange(C * H * W, dtype=torch.int32, device=dev).view(C, H, W), 0, C * H * W)
    if isinstance(feature_mask, (tuple, list)):
        raise NotImplementedError("feature_mask: a tuple of masks is not supported")
    m = feature_mask
    if not torch.is_tensor(m) or m.is_floating_point() or m.dtype == torch.bool:
        raise TypeError("feature_mask must be an integer tensor")
    while m.dim() > 2 and m.shape[0] == 1:
        m = m[0]
    if tuple(m.shape) not in ((H, W), (C, H, W)):
        raise NotImplementedError(f"feature_mask must be ({H}, {W}) or ({C}, {H}, {W}) (optionally with leading 1s), shared by the "
                                  f"batch; got {tuple(feature_mask.shape)}")
    lo, hi = int(m.min()), int(m.max())
    if lo < -2 ** 31 or hi >= 2 ** 31:
        raise ValueError("feature_mask ids must fit int32")
    return PreparedMask(m.to(dev, torch.int32).contiguous(), lo, hi - lo + 1)


def harness_patch_mask(img_hw, num_patches=NUM_PATCHES):
    """The reference's patch_mask (evaluatePerturbation.py:96-97) on the host: ids 0 .. num_patches^2 - 1, row-major patches of
    int(img_hw / num_patches) pixels."""
    side = int(img_hw / num_patches)
    if side * num_patches != img_hw:
        raise ValueError(f"fa: the {num_patches} x {num_patches} patch mask of {side}-pixel patches does not cover a {img_hw}-pixel image "
                         "(the reference's mask does not broadcast against it either)")
    ids = torch.arange(num_patches ** 2).reshape(num_patches, num_patches)
    return ids.repeat_interleave(side, dim=0).repeat_interleave(side, dim=1)


def _window_args(sliding_window_shapes, strides, x, name):
    """captum's (C, h, w) window and int / tuple / None strides -> ((h, w), (stride_h, stride_w))"""
    C = x.shape[1]
    win = sliding_window_shapes
    if isinstance(win, (tuple, list)) and win and isinstance(win[0], (tuple, list)):
        raise NotImplementedError(f"{name}: a tuple of window shapes (several inputs) is not supported")
    win = tuple(int(v) for v in win)
    if len(win) != 3:
        raise ValueError(f"{name}: sliding_window_shapes must be (C, h, w) for (B, C, H, W) inputs, got {win}")
    if win[0] != C:
        raise NotImplementedError(f"{name}: only windows spanning all {C} channels are supported, got {win}")
    if strides is None:
        st = win
    elif isinstance(strides, int):
        st = (strides,) * 3
    else:
        st = tuple(int(v) for v in strides)
        if len(st) != 3:
            raise ValueError(f"{name}: strides must be an int or one value per window dimension, got {strides}")
    if st[0] < 1:
        raise ValueError(f"{name}: strides must be >= 1")
    return win[1:], st[1:]


def _harness_map(samples, H, W, shared):
    """resize -> |sum over channels| of evaluatePerturbation.py:92,181 from the g x g samples (B, C, g, g) -> (B, H, W).  With one id
    plane for all channels the C planes are identical and |a + a + a| is the up-sample kernel's scale 3, abs (as the gc row)."""
    B, C, g, _ = samples.shape
    # g is the caller's: resize_bilinear is K3 while g <= H, W and the reference's antialiased resize beyond
    if shared and C <= 3:
        return K.resize_bilinear(samples[:, 0].contiguous(), H, W, scale=float(C), take_abs=True)
    return abs_channel_sum(K.resize_bilinear(samples.reshape(B * C, g, g), H, W).view(B, C, H, W))


def _run(x, model, tgt, n_total, fill, pass_size, streams, graphs):
    """-> (s0 (B,), scores (B, n_total)): the target logits of the inputs (one pass of B) and of every altered image (passes of
    `pass_size` rows of the flat list); `fill(first, n, out)` is the K26 launch."""
    B, dev, img_shape = x.shape[0], x.device, tuple(x.shape[1:])
    N = B * n_total
    rows_tgt = tgt.repeat_interleave(n_total).view(N, 1)
    scores = torch.empty(N, dtype=torch.float32, device=dev)
    eager = {}

    def pass_of(b):
        make = lambda: _ScorePass(model, b, img_shape, dev)  # noqa: E731
        if graphs:
            return _PASSES.get(model, dev, (b, img_shape), make)
        key = (threading.get_ident(), b)
        if key not in eager:
            eager[key] = make()
        return eager[key]

    def score(p):
        return (p.run() if graphs else p.eager())[0]

    p0 = pass_of(B)
    p0.x.copy_(x)
    p0.tgt.copy_(tgt.view(B, 1))
    s0 = score(p0).clone()

    def one_pass(lo, hi):
        p = pass_of(hi - lo)
        fill(lo, hi - lo, p.x)
        p.tgt.copy_(rows_tgt[lo:hi])
        scores[lo:hi].copy_(score(p))

    run_passes(dev, N, pass_size, one_pass, streams, kind=("ablation", id(model), int(pass_size), img_shape, bool(graphs)))
    ABLATION_COUNTS["rows"] += N
    return s0, scores.view(B, n_total)


def _results(attr, samples, H, W, shared, want_map, attribution):
    if want_map is None:
        return attr
    m = _harness_map(samples, H, W, shared)
    return (attr, m) if attribution else m


def feature_ablation_batch(x, model, targets, feature_mask, baseline=0, pass_size=PASS_SIZE, want_map=None, attribution=True, streams=1,
                           graphs=True):
    """captum's FeatureAblation attribution of B independent images: x (B, C, H, W) on a HIP device, `targets` one class index or
    one per image (int, list or tensor; a device tensor is not read back), `feature_mask` as `prepare_mask` takes it (shared by the
    images), `baseline` a number or a (C, H, W) tensor.  -> (B, C, H, W) device tensor: at every element of feature j,
    s0 - score(x with feature j replaced by the baseline); ids between the mask's minimum and maximum that occur nowhere still
    cost a forward, as in captum.
    `want_map=g`: additionally (or, with `attribution=False`, instead) the harness's (B, H, W) map |sum_c resize(downsize(attr))|
    (evaluatePerturbation.py:92-97, :181) with a g x g nearest-exact `downsize`.
    `pass_size`: rows of the flat list of altered images per classifier pass; `streams` > 1: the passes run on that many stream
    workers; `graphs`: replay each distinct pass size from a hipGraph."""
    x = check_input(x, "feature_ablation_batch")
    B, C, H, W = x.shape
    tgt = class_targets(targets, B, x.device, "feature_ablation_batch")
    base = _baseline(baseline, x, "feature_ablation_batch")
    pm = prepare_mask(feature_mask, x.shape, x.device)
    if want_map is None and not attribution:
        raise ValueError("feature_ablation_batch: nothing to return (want_map is None and attribution is False)")

    def fill(first, n, out):
        K.ablate_features(x, pm.ids, pm.id_min, pm.n_total, base, first, n, out=out)
    s0, scores = _run(x, model, tgt, pm.n_total, fill, pass_size, streams, graphs)
    attr, samples = K.ablation_finish_features(s0, scores, pm.ids, pm.id_min, (B, C, H, W), g=want_map, want_attr=attribution)
    return _results(attr, samples, H, W, pm.ids.dim() == 2, want_map, attribution)


def occlusion_batch(x, model, targets, sliding_window_shapes, strides=None, baseline=0, pass_size=PASS_SIZE, want_map=None,
                    attribution=True, streams=1, graphs=True):
    """captum's Occlusion attribution of B independent images: `sliding_window_shapes` (C, h, w) spanning all channels, `strides`
    an int (every dimension), a (c, h, w) tuple or None (= the window).  Windows are enumerated in captum's order (the row shift
    fastest), overhanging ones clipped to the image; -> (B, C, H, W): per element the sum of s0 - score(window k) over the windows
    covering it, ascending k, divided by their number.  The other arguments as `feature_ablation_batch`."""
    x = check_input(x, "occlusion_batch")
    B, C, H, W = x.shape
    tgt = class_targets(targets, B, x.device, "occlusion_batch")
    base = _baseline(baseline, x, "occlusion_batch")
    win, st = _window_args(sliding_window_shapes, strides, x, "occlusion_batch")
    ch, cw = K.window_counts(H, W, win, st)
    if want_map is None and not attribution:
        raise ValueError("occlusion_batch: nothing to return (want_map is None and attribution is False)")

    def fill(first, n, out):
        K.ablate_windows(x, win, st, base, first, n, out=out)
    s0, scores = _run(x, model, tgt, ch * cw, fill, pass_size, streams, graphs)
    attr, samples = K.ablation_finish_windows(s0, scores, win, st, (B, C, H, W), g=want_map, want_attr=attribution)
    return _results(attr, samples, H, W, True, want_map, attribution)


def _pass_size(perturbations_per_eval):
    n = int(perturbations_per_eval)
    if n < 1:
        raise ValueError("perturbations_per_eval must be >= 1")
    return PASS_SIZE if n == 1 else n        # captum's default of one altered image per call is exactly what this engine replaces


def _refuse(unsupported, name):
    if unsupported:                                   # additional_forward_args, show_progress, ...: captum arguments this path does not serve
        raise NotImplementedError(f"{name}: {', '.join(sorted(unsupported))} not supported on the HIP path")


class FeatureAblation:
    """captum.attr.FeatureAblation's call shape on the HIP path, for what the harness uses (evaluatePerturbation.py:171-173)."""

    def __init__(self, forward_func):
        self.forward_func = forward_func

    def attribute(self, inputs, baselines=None, target=None, feature_mask=None, perturbations_per_eval=1, **unsupported):
        """-> (B, C, H, W) device tensor.  Altered images are always batched (`perturbations_per_eval` above 1 sets the pass size);
        the attribution does not depend on it beyond the classifier's own rounding at another batch size."""
        _refuse(unsupported, "FeatureAblation.attribute")
        return feature_ablation_batch(inputs, self.forward_func, target, feature_mask, baseline=baselines,
                                      pass_size=_pass_size(perturbations_per_eval))


class Occlusion:
    """captum.attr.Occlusion's call shape on the HIP path, for what the harness uses (evaluatePerturbation.py:174-176)."""

    def __init__(self, forward_func):
        self.forward_func = forward_func

    def attribute(self, inputs, sliding_window_shapes, strides=None, baselines=None, target=None, perturbations_per_eval=1,
                  **unsupported):
        _refuse(unsupported, "Occlusion.attribute")
        return occlusion_batch(inputs, self.forward_func, target, sliding_window_shapes, strides, baseline=baselines,
                               pass_size=_pass_size(perturbations_per_eval))


def patch_captum():
    """Opt-in, and separate from gradcam.patch_captum (which touches LayerGradCam only): make `from captum.attr import
    FeatureAblation, Occlusion` -- evaluatePerturbation.py:43 -- resolve to the classes above.  Only these two names of an installed
    captum's `captum.attr` are rebound; its defining modules keep their own classes (captum's Occlusion derives from its
    FeatureAblation).  -> the (FeatureAblation, Occlusion) pair that was replaced, or None when captum is not importable."""
    try:
        import captum.attr as cattr
    except ImportError:
        return None
    old = (getattr(cattr, "FeatureAblation", None), getattr(cattr, "Occlusion", None))
    cattr.FeatureAblation, cattr.Occlusion = FeatureAblation, Occlusion
    return old
